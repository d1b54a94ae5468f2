#!/usr/bin/env python3
"""Interleaved A/B of two or more BUILDS of libtavb.so on the cfg3 shape: 10M x 1536 random fp16 rows, 1024 random queries, k = 32,
min_score 0, on one GPU, the builds taking turns (same box, same thermal state).

    cp typeagent_py_amd/libtavb.so typeagent_py_amd/libtavb_prev.so      (at the parent commit, after `make -C typeagent_py_amd/csrc`)
    python tools/library_ab.py [libtavb_prev.so libtavb.so ...]          (at the commit under test, after its own build; first = the baseline)

ONE PROCESS PER BUILD.  The binding opens the library RTLD_GLOBAL and the library's internal `namespace tavb` symbols have default
visibility: with two builds in one process the second one's calls into `tavb::launch_mfma_scan` and the like bind to the FIRST one's
definitions, and both engines launch the same kernels.  So this driver never touches the GPU; it starts one worker per build
(`--worker LIB`, TAVB_LIBRARY=LIB), each with its own copy of the corpus (30 GB) drawn from the same seed, and hands out turns over the
workers' pipes; a worker is idle while another runs.  Each worker reports the SHA-256 of the library file it has mapped and checks that no
other libtavb build is mapped in its process; the driver refuses to go on when two workers report the same hash.

After a warm-up turn the keys of every build are compared with the baseline's (SHA-256 over all 1024 x 32 keys).  Then AB_ROUNDS rounds of
AB_STEPS lookups per build, the starting build rotating per round; per-lookup wall time around search_device and a synchronise, board clock
and power sampled from hwmon during the turn (bench.py's HwmonSampler).  Then AB_ABL_ROUNDS rounds of the same with option mfma_ablate=258
(MFMA-only: no staging, no admissions; the keys are garbage): shipping / MFMA-only is the share of its own MFMA rate a build reaches.
Prints one line per turn and a JSON summary per build: median / min over the rounds, the round-to-round spread ((max - min) / median of
the round means), gain of the medians over the baseline, and whether the gain clears three times the larger of the two spreads.  With
AB_OUT=DIR also writes DIR/lib_ab_<AB_TAG>.json.  (profiles/r12_kloop_issue.md)"""
import hashlib, json, os, subprocess, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = int(os.environ.get("AB_ROWS", 10_000_000)); DIM = 1536; NQ = 1024; K = 32


def worker(lib_name):
    os.environ["TAVB_LIBRARY"] = lib_name
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import bench
    from typeagent_py_amd import _native

    say = lambda obj: (sys.stdout.write(json.dumps(obj) + "\n"), sys.stdout.flush())
    g = torch.Generator(device="cuda").manual_seed(1234)
    corpus = torch.empty((ROWS, DIM), dtype=torch.float16, device="cuda")
    for i in range(0, ROWS, 1 << 20):
        x = torch.randn((min(1 << 20, ROWS - i), DIM), generator=g, device="cuda")
        corpus[i:i + x.shape[0]] = (x / x.norm(dim=1, keepdim=True)).half()
    q = torch.randn((NQ, DIM), generator=g, device="cuda"); q = (q / q.norm(dim=1, keepdim=True)).contiguous()
    eng = _native.Engine(0)
    eng.set_corpus_tensor(corpus)
    out = torch.empty((NQ, K), dtype=torch.int64, device="cuda")
    mapped = sorted({ln.split()[-1] for ln in open("/proc/self/maps") if "libtavb" in ln})
    assert mapped == [_native.library_path()], f"{lib_name}: mapped {mapped}"
    say({"ready": lib_name, "sha256": hashlib.sha256(open(mapped[0], "rb").read()).hexdigest()})
    for line in sys.stdin:
        cmd = json.loads(line)
        if cmd["op"] == "quit":
            break
        eng.set_option("mfma_ablate", cmd.get("ablate", 0))
        torch.cuda.synchronize(); eng.synchronize()
        with bench.HwmonSampler(torch, 0) as hw:
            t = time.perf_counter()
            for _ in range(cmd["n"]):
                eng.search_device(q, K, 0.0, out_keys=out)
            eng.synchronize()
            ms = (time.perf_counter() - t) / cmd["n"] * 1e3
        rep = {"ms": ms, "tier": eng.get_option("last_tier"), "shape": eng.get_option("last_mfma_shape"), **(hw.summary() or {})}
        if cmd.get("keys"):
            rep["keys_sha256"] = hashlib.sha256(np.ascontiguousarray(out.cpu().numpy()).tobytes()).hexdigest()
        say(rep)
    eng.close()


def main():
    import numpy as np

    libs = sys.argv[1:] or ["libtavb_prev.so", "libtavb.so"]
    rounds = int(os.environ.get("AB_ROUNDS", 6)); per = int(os.environ.get("AB_STEPS", 8)); abl_rounds = int(os.environ.get("AB_ABL_ROUNDS", 2))
    procs = {}
    shas = {}

    def ask(lib, cmd=None):
        p = procs[lib]
        if cmd is not None:
            p.stdin.write(json.dumps(cmd) + "\n"); p.stdin.flush()
        while True:
            line = p.stdout.readline()
            if not line:
                raise SystemExit(f"worker {lib} ended (exit status {p.wait()})")
            if line.startswith("{"):
                return json.loads(line)

    try:
        for lib in libs:  # one after the other: the corpora are drawn on the GPU
            procs[lib] = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", lib], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
            ready = ask(lib)
            print(ready, flush=True)
            if ready["sha256"] in shas.values():
                raise SystemExit(f"{lib} is byte for byte another build of the list: nothing to compare")
            shas[lib] = ready["sha256"]
        hashes = {}
        for lib in libs:
            r = ask(lib, {"op": "run", "n": 3, "keys": True})
            hashes[lib] = r["keys_sha256"]
            print("warm-up", lib, r, flush=True)
        res = {lib: [] for lib in libs}; abl = {lib: [] for lib in libs}; hwm = {lib: [] for lib in libs}
        for r in range(rounds + abl_rounds):
            order = libs[r % len(libs):] + libs[:r % len(libs)]
            for lib in order:
                rep = ask(lib, {"op": "run", "n": per, "ablate": 258 if r >= rounds else 0})
                (abl if r >= rounds else res)[lib].append(rep["ms"])
                if r < rounds:
                    hwm[lib].append((rep.get("sclk_mhz"), rep.get("power_w")))
            print("round", r, "mfma-only" if r >= rounds else "shipping", {lib: round((abl if r >= rounds else res)[lib][-1], 3) for lib in libs}, flush=True)
    finally:
        for lib, p in procs.items():
            try:
                p.stdin.write(json.dumps({"op": "quit"}) + "\n"); p.stdin.flush()
            except Exception:
                pass
        for p in procs.values():
            try:
                p.wait(timeout=60)
            except Exception:
                p.kill()
    summ = {}
    for lib in libs:
        v = res[lib]
        med = lambda a: float(np.median([x for x in a if x is not None])) if any(x is not None for x in a) else None
        summ[lib] = {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "spread": float((np.max(v) - np.min(v)) / np.median(v)), "all": [round(x, 3) for x in v],
                     "sclk_mhz": med([h[0] for h in hwm[lib]]), "power_w": med([h[1] for h in hwm[lib]]), "keys_identical_to_baseline": hashes[lib] == hashes[libs[0]]}
        if abl[lib]:
            summ[lib]["mfma_only_ms"] = float(np.median(abl[lib]))
            summ[lib]["shipping_over_mfma_only"] = summ[lib]["mfma_only_ms"] / summ[lib]["median_ms"]
    base = summ[libs[0]]
    for lib in libs[1:]:
        s = summ[lib]
        s["gain_median"] = 1.0 - s["median_ms"] / base["median_ms"]
        s["bar"] = 3.0 * max(s["spread"], base["spread"])
        s["clears_bar"] = bool(s["gain_median"] > s["bar"])
    print(json.dumps(summ), flush=True)
    if os.environ.get("AB_OUT"):
        os.makedirs(os.environ["AB_OUT"], exist_ok=True)
        json.dump(summ, open(os.path.join(os.environ["AB_OUT"], f"lib_ab_{os.environ.get('AB_TAG', 'x')}.json"), "w"), indent=1)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--worker":
        worker(sys.argv[2])
    else:
        main()
