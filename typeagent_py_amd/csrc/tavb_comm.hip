// Row-sharded corpora: the RCCL binding of libtavb.so -- tavb_comm_*, tavb_search_allgather, tavb_allgather_merge and their large-k
// forms tavb_search_topk_allgather, tavb_allgather_merge_topk, and the top-messages forms tavb_search_top_messages_allgather,
// tavb_allgather_merge_top_messages.  The only file that
// includes RCCL's header (the context holds the communicator as an opaque pointer).  Host code only.

#include <dlfcn.h>
#include <rccl/rccl.h>  // types and prototypes only: the functions are resolved with dlsym (tavb_comm_init)

#include <chrono>
#include <mutex>
#include <thread>

#include "tavb_ctx.h"

using namespace tavb::host;

// ---- RCCL (resolved at run time: libtavb.so has no link-time dependency on librccl) -------------------------------------------
namespace {
ncclComm_t comm_of(const tavb_ctx* c) { return static_cast<ncclComm_t>(c->comm); }

struct Rccl {
  void* handle = nullptr;
  decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
  decltype(&ncclCommInitRank) CommInitRank = nullptr;
  decltype(&ncclCommDestroy) CommDestroy = nullptr;
  decltype(&ncclCommAbort) CommAbort = nullptr;  // (optional: only the timeout path needs it)
  decltype(&ncclAllGather) AllGather = nullptr;
  decltype(&ncclGetErrorString) GetErrorString = nullptr;
};
Rccl g_rccl;
std::once_flag g_rccl_once;
std::string g_rccl_error;

int load_rccl() {
  std::call_once(g_rccl_once, [] {
    // the copy the process already has (torch ships one with the same SONAME) before a fresh one from the ROCm tree
    const char* names[] = {"librccl.so.1", "librccl.so"};
    for (const char* n : names)
      if (!g_rccl.handle) g_rccl.handle = dlopen(n, RTLD_NOW | RTLD_NOLOAD | RTLD_GLOBAL);
    for (const char* n : names)
      if (!g_rccl.handle) g_rccl.handle = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
    if (!g_rccl.handle) {
      const char* e = dlerror();
      g_rccl_error = std::string("cannot load librccl.so.1: ") + (e ? e : "not found");
      return;
    }
    g_rccl.GetUniqueId = reinterpret_cast<decltype(g_rccl.GetUniqueId)>(dlsym(g_rccl.handle, "ncclGetUniqueId"));
    g_rccl.CommInitRank = reinterpret_cast<decltype(g_rccl.CommInitRank)>(dlsym(g_rccl.handle, "ncclCommInitRank"));
    g_rccl.CommDestroy = reinterpret_cast<decltype(g_rccl.CommDestroy)>(dlsym(g_rccl.handle, "ncclCommDestroy"));
    g_rccl.CommAbort = reinterpret_cast<decltype(g_rccl.CommAbort)>(dlsym(g_rccl.handle, "ncclCommAbort"));
    g_rccl.AllGather = reinterpret_cast<decltype(g_rccl.AllGather)>(dlsym(g_rccl.handle, "ncclAllGather"));
    g_rccl.GetErrorString = reinterpret_cast<decltype(g_rccl.GetErrorString)>(dlsym(g_rccl.handle, "ncclGetErrorString"));
    if (!g_rccl.GetUniqueId || !g_rccl.CommInitRank || !g_rccl.CommDestroy || !g_rccl.AllGather || !g_rccl.GetErrorString)
      g_rccl_error = "librccl.so.1 lacks one of ncclGetUniqueId / ncclCommInitRank / ncclCommDestroy / ncclAllGather / ncclGetErrorString";
  });
  if (!g_rccl_error.empty()) return fail(TAVB_E_UNSUPPORTED, "%s", g_rccl_error.c_str());
  return TAVB_OK;
}
static_assert(TAVB_COMM_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "the rendezvous id is RCCL's");

#define TAVB_RCCL(expr)                                                                                             \
  do {                                                                                                              \
    ncclResult_t r__ = (expr);                                                                                      \
    if (r__ != ncclSuccess) return fail(TAVB_E_HIP, "%s failed: %s (%s:%d)", #expr, g_rccl.GetErrorString(r__), __FILE__, __LINE__); \
  } while (0)

}  // namespace

// tavb_synchronize with an exchange in flight and "comm_timeout_ms" set: polls the stream; when the deadline passes (a peer never joined the
// all-gather, or died in it) the communicator is ABORTED -- ncclCommAbort makes the collective's kernel return, so the stream drains -- and the
// context is left without one (tavb_comm_init again to rejoin): TAVB_E_TIMEOUT, never a process stuck in a collective for ever.
int tavb::host::comm_wait_or_abort(tavb_ctx* c) {
  const auto t0 = std::chrono::steady_clock::now();
  const auto deadline = t0 + std::chrono::milliseconds(c->comm_timeout_ms);
  int polls = 0;
  for (;;) {
    const hipError_t e = hipStreamQuery(c->stream);
    if (e == hipSuccess) {
      c->comm_inflight = false;
      return TAVB_OK;
    }
    if (e != hipErrorNotReady) return fail(TAVB_E_HIP, "hipStreamQuery failed: %s", hipGetErrorString(e));
    if (std::chrono::steady_clock::now() >= deadline) break;
    if (++polls > 2000) std::this_thread::sleep_for(std::chrono::microseconds(50));  // (the first polls spin: a lookup of a small shard is that short)
  }
  ncclComm_t comm = comm_of(c);
  c->comm = nullptr;
  c->comm_rank = 0;
  c->comm_world = 1;
  c->comm_inflight = false;
  const long long waited = std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t0).count();
  if (g_rccl.CommAbort) (void)g_rccl.CommAbort(comm);
  (void)hipStreamSynchronize(c->stream);  // (drains once the aborted collective has let go of the stream)
  return fail(TAVB_E_TIMEOUT, "the exchange did not complete within %lld ms (option comm_timeout_ms): a peer never joined the all-gather; "
              "the communicator was aborted -- tavb_comm_init to rejoin", waited);
}

extern "C" {

int tavb_comm_unique_id(void* out_id) {
  if (!out_id) return fail(TAVB_E_INVALID, "null out_id");
  if (int rc = load_rccl()) return rc;
  ncclUniqueId id;
  TAVB_RCCL(g_rccl.GetUniqueId(&id));
  memcpy(out_id, id.internal, TAVB_COMM_ID_BYTES);
  return TAVB_OK;
}

int tavb_comm_init(tavb_ctx* c, const void* id_bytes, int32_t rank, int32_t world) {
  if (int rc = check_ctx(c)) return rc;
  if (!id_bytes) return fail(TAVB_E_INVALID, "null id");
  if (world < 1 || rank < 0 || rank >= world) return fail(TAVB_E_INVALID, "rank %d out of range for world %d", rank, world);
  if (c->comm) return fail(TAVB_E_INVALID, "this context already has a communicator (tavb_comm_destroy first)");
  if (int rc = load_rccl()) return rc;
  DeviceGuard guard(c->device);
  ncclUniqueId id;
  memcpy(id.internal, id_bytes, TAVB_COMM_ID_BYTES);
  // the exchange buffers come first: a rank that cannot have them fails HERE, in a collective every rank is still free to fail in, and no
  // exchange of up to comm_reserve_keys keys allocates anything afterwards (8 MiB + world x 8 MiB at the default)
  if (int rc = c->d_xlocal.reserve((size_t)c->comm_reserve_keys * sizeof(u64_t))) return rc;
  if (int rc = c->d_gather.reserve((size_t)c->comm_reserve_keys * sizeof(u64_t) * world)) return rc;
  ncclComm_t comm = nullptr;
  TAVB_RCCL(g_rccl.CommInitRank(&comm, world, id, rank));
  c->comm = comm;
  c->comm_rank = rank;
  c->comm_world = world;
  c->comm_chunk_keys = c->comm_reserve_keys;
  c->comm_inflight = false;
  return TAVB_OK;
}

int tavb_comm_destroy(tavb_ctx* c) {
  if (!c || !c->comm) return TAVB_OK;
  DeviceGuard guard(c->device);
  (void)hipStreamSynchronize(c->stream);
  ncclComm_t comm = comm_of(c);
  c->comm = nullptr;
  c->comm_rank = 0;
  c->comm_world = 1;
  if (g_rccl.CommDestroy) TAVB_RCCL(g_rccl.CommDestroy(comm));
  return TAVB_OK;
}

}  // extern "C"

// local [nq, k] lists (device; nullptr = this rank FAILED: it sends TAVB_KEY_PEER_FAILED in every slot) -> ncclAllGather on the context's
// stream -> merge kernel -> out_keys [nq, k].  Nothing in front of an all-gather allocates: the lists travel through the buffers tavb_comm_init reserved, in chunks
// of whole queries when they hold more than comm_reserve_keys keys.  Every rank makes the same call and cuts by the value tavb_comm_init
// stored (comm_chunk_keys), so every rank cuts the same chunks.  The merge is the one difference between the families of collective calls:
// kMergeFused, the register merge (k up to TAVB_MAX_FUSED_K); kMergeLong, the merge of tavb_topk.hip (any k up to TAVB_MAX_LARGE_K, up to 64
// ranks); kMergeMessages, the same shapes for keys that carry MESSAGE ordinals -- one maximum per message, then the top-messages selection
// (merge_top_messages_impl over the context's n_messages).  That merge has workspaces of its own (d_msg_best, d_topk: no larger than the
// rank's own lookup reserved, plan_top_messages), reserved behind the chunk's all-gather; a rank whose merge fails all the same stops
// merging but still joins the all-gathers of EVERY later chunk -- the peers are never left waiting -- and returns its error at the end.
enum MergeKind { kMergeFused, kMergeLong, kMergeMessages };

static int exchange_and_merge(tavb_ctx* c, const u64_t* local, int32_t nq, int32_t k, MergeKind merge, tavb_key* out_keys) {
  const int qc = (int)std::min<int64_t>(nq, std::max<int64_t>(1, c->comm_chunk_keys / k));  // queries per chunk
  if ((size_t)qc * k * sizeof(u64_t) * c->comm_world > c->d_gather.cap || (size_t)qc * k * sizeof(u64_t) > c->d_xlocal.cap)
    return fail(TAVB_E_INVALID, "the exchange buffers of this communicator are gone (tavb_comm_init reserves them)");
  u64_t* gathered = reinterpret_cast<u64_t*>(c->d_gather.ptr);
  if (!local) (void)hipMemsetAsync(c->d_xlocal.ptr, 0xFF, (size_t)qc * k * sizeof(u64_t), c->stream);
  if (c->comm_stall_ms > 0) {  // fault injection: one shot
    (void)tavb::launch_stall((int)c->comm_stall_ms, c->stream);
    c->comm_stall_ms = 0;
  }
  c->comm_inflight = true;
  int rc_merge = TAVB_OK;
  std::string merge_error;
  for (int q0 = 0; q0 < nq; q0 += qc) {
    const int qn = std::min(qc, nq - q0);
    const u64_t* src = local ? local + (size_t)q0 * k : reinterpret_cast<const u64_t*>(c->d_xlocal.ptr);
    {
      Timed t(c, TAVB_KERNEL_EXCHANGE);
      TAVB_RCCL(g_rccl.AllGather(src, gathered, (size_t)qn * k, ncclUint64, comm_of(c), c->stream));
    }
    u64_t* out = reinterpret_cast<u64_t*>(out_keys) + (size_t)q0 * k;
    if (merge == kMergeMessages) {
      if (rc_merge != TAVB_OK) continue;  // (this rank's merge has failed: it only keeps the collectives company)
      if ((rc_merge = c->h_topk_rounds.reserve((size_t)nq * sizeof(int32_t))) == TAVB_OK)
        rc_merge = merge_top_messages_impl(c, gathered, c->comm_world, qn, k, /*query_major=*/false, c->n_messages, out,
                                           reinterpret_cast<int32_t*>(c->h_topk_rounds.ptr) + q0);
      if (rc_merge != TAVB_OK) merge_error = g_last_error;
      continue;
    }
    Timed t(c, TAVB_KERNEL_MERGE);
    hipError_t e = merge == kMergeLong ? tavb::launch_merge_topk(gathered, c->comm_world, qn, k, /*query_major=*/false, out, c->stream)
                                       : tavb::launch_merge(gathered, c->comm_world, qn, k, /*query_major=*/false, out, c->stream);
    if (e != hipSuccess) return fail(TAVB_E_HIP, "merge launch failed: %s", hipGetErrorString(e));
  }
  if (rc_merge != TAVB_OK) {
    g_last_error = merge_error;
    return rc_merge;
  }
  if (merge == kMergeMessages) c->topk_rounds_pending = nq;  // ("last_topk_refine": the merge's rounds, at the next tavb_synchronize)
  return TAVB_OK;
}

// The collective lookups after their argument checks: everything that can fail on ONE rank -- the state of its shard, an allocation, a
// launch -- still joins the collectives, with TAVB_KEY_PEER_FAILED lists, so that the peers are never left waiting in ncclAllGather for a
// rank that has returned an error to its caller.  Lists of up to comm_reserve_keys keys live in the buffer tavb_comm_init reserved: no
// allocation between here and the all-gather.  `search(local)` enqueues this shard's lookup into local [nq, k] and returns its status -- the
// workspaces it reserves on the way are part of it: a failure there joins the exchange like any other.
template <class Search>
static int search_exchange_merge(tavb_ctx* c, int32_t nq, int32_t k, MergeKind merge, tavb_key* out_keys, Search&& search) {
  DeviceGuard guard(c->device);
  const size_t list_keys = (size_t)nq * k;
  int rc_local = TAVB_OK;
  u64_t* local = nullptr;
  if ((rc_local = require_corpus(c)) != TAVB_OK) {
  } else if ((rc_local = check_key_ordinals(c, /*device_resident=*/true)) != TAVB_OK) {
  } else if (list_keys <= (size_t)c->comm_chunk_keys && list_keys * sizeof(u64_t) <= c->d_xlocal.cap) local = reinterpret_cast<u64_t*>(c->d_xlocal.ptr);
  else if (c->comm_fail_alloc) rc_local = fail(TAVB_E_NOMEM, "injected failure of the list allocation (option comm_fail_alloc)");
  else if ((rc_local = c->d_local.reserve(list_keys * sizeof(u64_t))) == TAVB_OK) local = reinterpret_cast<u64_t*>(c->d_local.ptr);
  if (rc_local != TAVB_OK) {
  } else if (c->comm_fail_rank >= 0 && c->comm_fail_rank == c->comm_rank) {  // fault injection (option "comm_fail_rank"): what a failed launch / allocation inside the local search looks like
    rc_local = fail(TAVB_E_HIP, "injected failure of the local search on rank %d (option comm_fail_rank)", c->comm_rank);
  } else if (c->rows == 0) {  // an empty shard still takes part in the collectives
    const hipError_t e = hipMemsetAsync(local, 0, list_keys * sizeof(u64_t), c->stream);
    if (e != hipSuccess) rc_local = fail(TAVB_E_HIP, "hipMemsetAsync failed: %s", hipGetErrorString(e));
  } else {
    rc_local = search(local);
  }
  // a failed rank's lists = TAVB_KEY_PEER_FAILED (all bits set) in every slot: it sorts above every real key, so it leads every merged list on
  // EVERY rank -- the peers' answers would silently miss this shard otherwise; tavb_decode_keys turns it into TAVB_E_PEER
  const std::string local_error = rc_local != TAVB_OK ? g_last_error : std::string();
  const int rc_x = exchange_and_merge(c, rc_local == TAVB_OK ? local : nullptr, nq, k, merge, out_keys);
  if (rc_local != TAVB_OK) {
    g_last_error = local_error;
    return rc_local;
  }
  return rc_x;
}

static bool collective(const tavb_ctx* c) { return c->comm && !(c->comm_world == 1 && !c->comm_force); }

// argument errors of the large-k collectives that every rank makes alike
static int check_long_lists(const tavb_ctx* c, int32_t nq, int32_t k) {
  if (k < 1 || k > TAVB_MAX_LARGE_K) return fail(TAVB_E_INVALID, "k must be 1 .. %d (got %d)", TAVB_MAX_LARGE_K, k);
  if (nq < 1) return fail(TAVB_E_INVALID, "nq must be >= 1");
  if (collective(c) && k > c->comm_chunk_keys)
    return fail(TAVB_E_INVALID, "one list of k=%d keys does not fit the exchange buffers (option comm_reserve_keys = %lld, read by tavb_comm_init)", k,
                (long long)c->comm_chunk_keys);
  if (collective(c) && c->comm_world > 64) return fail(TAVB_E_UNSUPPORTED, "the merge of lists beyond %d keys takes up to 64 ranks", TAVB_MAX_FUSED_K);
  return TAVB_OK;
}

extern "C" {

int tavb_search_allgather(tavb_ctx* c, const float* dev_queries, int32_t nq, int32_t k, float min_score, tavb_key* out_keys) {
  // argument errors every rank makes alike (the ranks make the same call) return at once ...
  if (int rc = check_ctx(c)) return rc;
  if (k < 1) return fail(TAVB_E_INVALID, "k must be >= 1 (got %d)", k);
  if (k > TAVB_MAX_FUSED_K)
    return fail(TAVB_E_UNSUPPORTED, "k=%d exceeds the fused-select limit %d; page with tavb_search_after / tavb_search_subset_after", k, TAVB_MAX_FUSED_K);
  if (nq < 1) return fail(TAVB_E_INVALID, "nq must be >= 1");
  if (!dev_queries || !out_keys) return fail(TAVB_E_INVALID, "null argument");
  if (!collective(c)) return tavb_search_device(c, dev_queries, nq, k, min_score, out_keys);
  // ... everything else joins the exchange (search_exchange_merge)
  const std::vector<float> ms((size_t)nq, min_score);
  return search_exchange_merge(c, nq, k, kMergeFused, out_keys, [&](u64_t* local) {
    return tavb_search_device_dispatch(c, dev_queries, nq, k, ms.data(), (uint32_t)c->ordinal_base, local);
  });
}

int tavb_search_topk_allgather(tavb_ctx* c, const float* dev_queries, int32_t nq, int32_t k, const float* min_scores, tavb_key* out_keys) {
  if (int rc = check_ctx(c)) return rc;
  if (int rc = check_long_lists(c, nq, k)) return rc;
  if (!dev_queries || !min_scores || !out_keys) return fail(TAVB_E_INVALID, "null argument");
  if (!collective(c)) return tavb_search_topk_device(c, dev_queries, nq, k, min_scores, nullptr, 0, out_keys);
  return search_exchange_merge(c, nq, k, kMergeLong, out_keys, [&](u64_t* local) {
    return search_topk_async(c, dev_queries, nq, k, min_scores, nullptr, c->rows, (uint32_t)c->ordinal_base, local);
  });
}

static int allgather_merge_impl(tavb_ctx* c, const tavb_key* dev_local_keys, int32_t nq, int32_t k, MergeKind merge, tavb_key* out_keys) {
  if (!dev_local_keys || !out_keys) return fail(TAVB_E_INVALID, "null argument");
  DeviceGuard guard(c->device);
  if (!collective(c)) {
    if (reinterpret_cast<const void*>(dev_local_keys) != reinterpret_cast<const void*>(out_keys))
      TAVB_HIP(hipMemcpyAsync(out_keys, dev_local_keys, (size_t)nq * k * sizeof(u64_t), hipMemcpyDefault, c->stream));
    return TAVB_OK;
  }
  return exchange_and_merge(c, reinterpret_cast<const u64_t*>(dev_local_keys), nq, k, merge, out_keys);
}

int tavb_allgather_merge(tavb_ctx* c, const tavb_key* dev_local_keys, int32_t nq, int32_t k, tavb_key* out_keys) {
  if (int rc = check_ctx(c)) return rc;
  if (nq < 1 || k < 1 || k > TAVB_MAX_FUSED_K) return fail(TAVB_E_INVALID, "bad list shape");
  return allgather_merge_impl(c, dev_local_keys, nq, k, kMergeFused, out_keys);
}

int tavb_allgather_merge_topk(tavb_ctx* c, const tavb_key* dev_local_keys, int32_t nq, int32_t k, tavb_key* out_keys) {
  if (int rc = check_ctx(c)) return rc;
  if (int rc = check_long_lists(c, nq, k)) return rc;
  return allgather_merge_impl(c, dev_local_keys, nq, k, kMergeLong, out_keys);
}

// argument errors of the top-messages collectives that every rank makes alike: check_long_lists, and the context's n_messages -- every rank
// sets the same one (tavb_set_row_messages), a rank without rows included; 0 means no map was ever set
static int check_message_lists(const tavb_ctx* c, int32_t nq, int32_t k) {
  if (int rc = check_long_lists(c, nq, k)) return rc;
  if (c->n_messages == 0) return fail(TAVB_E_NO_CORPUS, "no row -> message map set (call tavb_set_row_messages first, with the same n_messages on every rank)");
  if (c->n_messages >= 0x7FFFFFFFll) return fail(TAVB_E_UNSUPPORTED, "top-messages keys hold message ordinals: n_messages must be < 2^31 - 1");
  return TAVB_OK;
}

int tavb_search_top_messages_allgather(tavb_ctx* c, const float* dev_queries, int32_t nq, int32_t k, const float* min_scores, const int32_t* dev_rows,
                                       int64_t n_rows, tavb_key* out_keys) {
  // argument errors every rank makes alike return at once ...
  if (int rc = check_ctx(c)) return rc;
  if (int rc = check_message_lists(c, nq, k)) return rc;
  if (!dev_queries || !min_scores || !out_keys) return fail(TAVB_E_INVALID, "null argument");
  if (!collective(c)) return tavb_search_top_messages_device(c, dev_queries, nq, k, min_scores, dev_rows, n_rows, out_keys);
  // ... everything else -- the row list's shape and a map that does not cover this rank's shard among it -- joins the exchange
  return search_exchange_merge(c, nq, k, kMergeMessages, out_keys, [&](u64_t* local) {
    bool empty = false;
    if (int rc = check_top_messages_args(c, k, dev_rows, n_rows, &empty)) return rc;
    c->topk_rounds_pending = 0;
    if (empty) return fill_empty_keys(c, local, (int64_t)nq * k);  // (this rank's part of the mask holds no row)
    if (int rc = c->h_topk_rounds.reserve((size_t)nq * sizeof(int32_t))) return rc;
    return search_top_messages_impl(c, dev_queries, nq, k, min_scores, dev_rows, n_rows, local, reinterpret_cast<int32_t*>(c->h_topk_rounds.ptr));
  });
}

int tavb_allgather_merge_top_messages(tavb_ctx* c, const tavb_key* dev_local_keys, int32_t nq, int32_t k, tavb_key* out_keys) {
  if (int rc = check_ctx(c)) return rc;
  if (int rc = check_message_lists(c, nq, k)) return rc;
  return allgather_merge_impl(c, dev_local_keys, nq, k, kMergeMessages, out_keys);
}

}  // extern "C"
