// pt_dist.cpp — the native multi-GPU step loop (pt_dist_*): the
// tile split's frames with the RCCL gather issued from C++, so a run of frames
// costs no Python per frame.
// bench.py's Python step (render_packed + torch.distributed.gather + stream
// switches) costs ~40-50 us of host time per frame, more than the ~40-us GPU
// step of a 1/8 box.obj share; here one frame is a render_packed launch, two
// event operations and one grouped send/recv.  The launches are the core's
// (pt_api.cpp render_impl, relaunch: pt_context.h).
#include <dlfcn.h>
#include <rccl/rccl.h>   // types only: the functions are resolved at run time (rccl_api)
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <thread>
#include <vector>

#include "pt_context.h"

// Native multi-GPU step loop state (pt_dist_*): an RCCL communicator of its
// own, a high-priority stream for the gathers, two render streams (frames
// alternate), and double-buffered send / receive slots.
constexpr int kDistStreams = 3;                 // render streams: frames k, k+1, .. in flight
constexpr int kDistSets = 2 * kDistStreams;     // frame k uses buffer set k % (2 D) (see pt_dist_run)
struct DistState {
  ncclComm_t comm = nullptr;
  int nranks = 0, rank = 0;
  int comm_count = -1;   // ncclCommCount of the communicator (-1: not reported by the library)
  hipStream_t comm_stream = nullptr;
  hipStream_t streams[kDistStreams] = {};
  hipStream_t own[kDistStreams + 1] = {};   // created here: render streams, then the gather stream
                                            // (pt_dist_set_streams may override)
  hipEvent_t render_done[kDistSets] = {}, gather_done[kDistSets] = {};
  hipEvent_t entry[kDistStreams + 1] = {};  // pt_dist_run's entry barrier: each stream's last work
  float* send[kDistStreams] = {};        // non-root ranks: frame k's live items (k % D)
  float* recv[kDistSets] = {};           // root: one slot per rank of the partition; slot 0 its own
  float* ingest = nullptr;               // emulated root: stand-in for the other ranks' slots
  size_t slot_floats = 0, cap_floats = 0;
  std::vector<float> layout_key;         // frame_key of the layout the slots were sized for
  // root: frame buffers that hold a whole assembled frame of a layout (its
  // culled items' constant (0,0,0,1) included); later frames of that layout
  // rebuild only their live items there (the culled bytes are the same)
  std::vector<std::pair<const void*, std::vector<float>>> assembled;
  bool ready = false;
  bool caller_streams = false;           // pt_dist_set_streams gave render streams (then at most 2)
};

namespace {
struct RcclApi {
  void* h = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommCount)(ncclComm_t, int*) = nullptr;   // optional (the tests' stand-in may lack it)
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*CommAbort)(ncclComm_t) = nullptr;
  ncclResult_t (*GroupStart)() = nullptr;
  ncclResult_t (*GroupEnd)() = nullptr;
  ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
};
// RCCL is loaded only when the multi-GPU loop is used: the one already in
// the process (torch's) if there is one, else the system's.  PT_RCCL_LIB
// names another library with the same nine entry points instead, and then
// only that one is tried (the tests' one-GPU stand-in, tests/dist_shim.cpp,
// which moves the point-to-point bytes between processes sharing a device).
const RcclApi* rccl_api() {
  static RcclApi api;
  static bool tried = false;
  if (!tried) {
    tried = true;
    const char* alt = getenv("PT_RCCL_LIB");
    void* h = nullptr;
    if (alt && *alt) {
      h = dlopen(alt, RTLD_NOW | RTLD_LOCAL);
    } else {
      h = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);
      if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
      if (!h) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    }
    if (h) {
      api.GetUniqueId = (decltype(api.GetUniqueId))dlsym(h, "ncclGetUniqueId");
      api.CommInitRank = (decltype(api.CommInitRank))dlsym(h, "ncclCommInitRank");
      api.CommCount = (decltype(api.CommCount))dlsym(h, "ncclCommCount");
      api.CommDestroy = (decltype(api.CommDestroy))dlsym(h, "ncclCommDestroy");
      api.CommAbort = (decltype(api.CommAbort))dlsym(h, "ncclCommAbort");
      api.GroupStart = (decltype(api.GroupStart))dlsym(h, "ncclGroupStart");
      api.GroupEnd = (decltype(api.GroupEnd))dlsym(h, "ncclGroupEnd");
      api.Send = (decltype(api.Send))dlsym(h, "ncclSend");
      api.Recv = (decltype(api.Recv))dlsym(h, "ncclRecv");
      api.GetErrorString = (decltype(api.GetErrorString))dlsym(h, "ncclGetErrorString");
      if (api.GetUniqueId && api.CommInitRank && api.CommDestroy && api.CommAbort && api.GroupStart && api.GroupEnd && api.Send &&
          api.Recv && api.GetErrorString)
        api.h = h;
    }
  }
  return api.h ? &api : nullptr;
}
#define PT_NCCL(call)                                                                                   \
  do {                                                                                                  \
    ncclResult_t r_ = (call);                                                                           \
    if (r_ != ncclSuccess) return fail(PT_ERR_HIP, std::string(#call ": ") + R->GetErrorString(r_));    \
  } while (0)

// Slot size and buffers for the layout of the last rendered frame (c->last).
int dist_layout(pt_context* c) {
  DistState* d = c->dist;
  std::vector<float> key;
  frame_key(c, c->last, &key);
  // (the root has no send slots: its layout is valid once any buffer was
  // sized for it; testing send[0] made the root rebuild every rank's item
  // lists on every call, ~0.45 ms of host time per call at N = 8)
  if (key == d->layout_key && d->cap_floats > 0) return PT_OK;
  size_t live_max = 0;
  std::vector<int> live, culled;
  for (int r = 0; r < c->nranks; ++r) {
    item_lists(c->last, part_of(c, r), &live, &culled);
    live_max = std::max(live_max, live.size());
  }
  const size_t slot = std::max<size_t>(4, live_max * (size_t)(256 / c->last.spl) * 4);
  const size_t nslots = (size_t)c->nranks;   // the partition's ranks (emulation: > d->nranks)
  if (slot > d->cap_floats) {
    for (int b = 0; b < kDistStreams; ++b)
      for (hipStream_t s : {d->streams[b], d->comm_stream}) PT_HIP(hipStreamSynchronize(s));
    for (int b = 0; b < kDistStreams; ++b) dev_free(d->send[b]);
    for (int b = 0; b < kDistSets; ++b) dev_free(d->recv[b]);
    dev_free(d->ingest);
    d->cap_floats = 0;
    for (int b = 0; b < kDistStreams && d->rank != 0; ++b) {
      PT_HIP(hipMalloc((void**)&d->send[b], slot * sizeof(float)));
      PT_HIP(hipMemset(d->send[b], 0, slot * sizeof(float)));
    }
    for (int b = 0; b < kDistSets && d->rank == 0; ++b) {
      PT_HIP(hipMalloc((void**)&d->recv[b], nslots * slot * sizeof(float)));
      PT_HIP(hipMemset(d->recv[b], 0, nslots * slot * sizeof(float)));
    }
    if (d->nranks == 1 && nslots > 1) {
      PT_HIP(hipMalloc((void**)&d->ingest, (nslots - 1) * slot * sizeof(float)));
      PT_HIP(hipMemset(d->ingest, 0, (nslots - 1) * slot * sizeof(float)));
    }
    d->cap_floats = slot;
  }
  d->slot_floats = slot;
  d->layout_key = key;
  return PT_OK;
}
}  // namespace

int dist_synchronize(pt_context* c) {
  for (hipStream_t s : {c->dist->streams[0], c->dist->streams[1], c->dist->comm_stream})
    if (s) PT_HIP(hipStreamSynchronize(s));
  return PT_OK;
}

extern "C" {

int pt_dist_unique_id(void* id, size_t id_bytes) {
  if (!id || id_bytes < sizeof(ncclUniqueId)) return fail(PT_ERR_INVALID, "id buffer must hold 128 bytes");
  const RcclApi* R = rccl_api();
  if (!R) return fail(PT_ERR_UNSUPPORTED, "RCCL (librccl.so.1) could not be loaded");
  ncclUniqueId u;
  PT_NCCL(R->GetUniqueId(&u));
  memcpy(id, &u, sizeof u);
  return PT_OK;
}

int pt_dist_init(pt_context* c, const void* id, int nranks, int rank) {
  PT_SINGLE(c, "pt_dist_init");
  if (!c || !id) return fail(PT_ERR_INVALID, "null argument");
  const bool emulated = nranks == 1 && rank == 0 && c->rank == 0 && c->nranks > 1;
  if (!emulated && (nranks != c->nranks || rank != c->rank))
    return fail(PT_ERR_INVALID, "pt_dist_init: set the same partition first (pt_set_partition / _slots)");
  const RcclApi* R = rccl_api();
  if (!R) return fail(PT_ERR_UNSUPPORTED, "RCCL (librccl.so.1) could not be loaded");
  if (c->dist) pt_dist_finalize(c);
  PT_HIP(hipSetDevice(c->device));
  DistState* d = new DistState();
  c->dist = d;
  d->nranks = nranks;
  d->rank = rank;
  int lo = 0, hi = 0;
  PT_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));
  PT_HIP(hipStreamCreateWithPriority(&d->own[kDistStreams], hipStreamNonBlocking, hi));   // gathers take CUs first
  // the two render streams at the least priority: the HIP runtime gives each
  // priority its own pool of GPU_MAX_HW_QUEUES hardware queues, so these two
  // get a queue each instead of sharing one with the process's other streams
  // (two frames on one queue do not overlap)
  for (int b = 0; b < kDistStreams; ++b) {
    PT_HIP(hipStreamCreateWithPriority(&d->own[b], hipStreamNonBlocking, lo));
    d->streams[b] = d->own[b];
  }
  d->comm_stream = d->own[kDistStreams];
  for (int b = 0; b < kDistSets; ++b) {
    PT_HIP(hipEventCreateWithFlags(&d->render_done[b], hipEventDisableTiming));
    PT_HIP(hipEventCreateWithFlags(&d->gather_done[b], hipEventDisableTiming));
  }
  for (hipEvent_t& e : d->entry) PT_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  ncclUniqueId u;
  memcpy(&u, id, sizeof u);
  PT_NCCL(R->CommInitRank(&d->comm, nranks, u, rank));
  if (R->CommCount) {
    int cnt = -1;
    if (R->CommCount(d->comm, &cnt) == ncclSuccess) d->comm_count = cnt;
  }
  d->ready = true;
  return PT_OK;
}

int pt_dist_info(pt_context* c, int* comm_ranks, int* nranks, int* rank) {
  PT_SINGLE(c, "pt_dist_info");
  if (!c || !c->dist) return fail(PT_ERR_INVALID, "pt_dist_info: no communicator (pt_dist_init)");
  if (comm_ranks) *comm_ranks = c->dist->comm_count;
  if (nranks) *nranks = c->dist->nranks;
  if (rank) *rank = c->dist->rank;
  return PT_OK;
}

// Whether frame buffer `frame` already holds a whole assembled frame of the
// layout `key` (its culled items' constant included).
static bool dist_assembled(const DistState* d, const void* frame, const std::vector<float>& key) {
  for (const auto& e : d->assembled)
    if (e.first == frame) return e.second == key;
  return false;
}
static void dist_mark_assembled(DistState* d, const void* frame, const std::vector<float>& key) {
  for (auto& e : d->assembled)
    if (e.first == frame) {
      e.second = key;
      return;
    }
  d->assembled.push_back({frame, key});
}

int pt_dist_run(pt_context* c, uint32_t n_batches, int n_frames, int n_streams, void* frames, int n_frame_bufs) {
  PT_SINGLE(c, "pt_dist_run");
  if (!c) return fail(PT_ERR_INVALID, "null context");
  if (c->opt_moments) return fail(PT_ERR_UNSUPPORTED, "PT_OPT_MOMENTS: not with pt_dist_run");
  DistState* d = c->dist;
  if (!d || !d->ready) return fail(PT_ERR_INVALID, "pt_dist_run: no communicator (pt_dist_init)");
  if (n_frames < 0 || n_batches == 0) return fail(PT_ERR_INVALID, "pt_dist_run: bad frame or batch count");
  if (d->rank == 0 && (!frames || n_frame_bufs < 1 || (((uintptr_t)frames) & 15)))
    return fail(PT_ERR_INVALID, "pt_dist_run: the root needs 16-B aligned frame buffers");
  if (n_streams < 1 || n_streams > kDistStreams) return fail(PT_ERR_INVALID, "pt_dist_run: 1 to 3 streams");
  if (d->caller_streams && n_streams > 2)
    return fail(PT_ERR_INVALID, "pt_dist_run: 3 streams with caller render streams (pt_dist_set_streams sets two)");
  const bool emulated = d->nranks == 1 && c->nranks > 1;
  if ((d->nranks != c->nranks && !emulated) || d->rank != c->rank)
    return fail(PT_ERR_INVALID, "partition changed since pt_dist_init");
  if (!c->last_valid) return fail(PT_ERR_INVALID, "pt_dist_run: render one frame with pt_render first (item layout)");
  const RcclApi* R = rccl_api();
  PT_HIP(hipSetDevice(c->device));
  {
    const int rc = dist_layout(c);
    if (rc) return rc;
  }
  const size_t slot = d->slot_floats;
  const size_t frame_f = (size_t)c->width * c->height * 4;
  hipStream_t saved = c->stream;
  int rc = PT_OK;
  // D = max(2, streams) frames in flight.  Frame k runs on stream k % S
  // with buffer set k % 2D.  Its launch (pt_render_packed) writes this rank's
  // live items -- on the root straight into its own slot of receive set
  // k % 2D, elsewhere into send slot k % D -- and, on the root, assembles
  // frame k-D from receive set (k-D) % 2D, after waiting for that frame's
  // gather.  Hazards: the gather of frame k (comm stream, after frame k's
  // launch) overwrites set k % 2D, which frame k-D's launch read -- earlier
  // on frame k's own stream (S divides D: S = 1 or D); a send slot is read by
  // the gather of frame k-D, which frame k's launch waits for.
  const int D = std::max(2, n_streams), nsets = 2 * D;
  // Those hazards hold within a call.  Across calls, frame k < D of this call
  // has no gather_done to wait for: a previous call's last sends (comm stream)
  // may still read send slot k % D, and its trailing assemblies (other render
  // streams) may still write the frame buffers.  So every render stream
  // starts behind every stream's last work of the previous call.
  {
    hipStream_t all[kDistStreams + 1];
    for (int s = 0; s < kDistStreams; ++s) all[s] = d->streams[s];
    all[kDistStreams] = d->comm_stream;
    for (int s = 0; s <= kDistStreams; ++s) PT_HIP(hipEventRecord(d->entry[s], all[s]));
    for (int s = 0; s < n_streams; ++s)
      for (int e = 0; e <= kDistStreams; ++e)
        if (all[e] != d->streams[s]) PT_HIP(hipStreamWaitEvent(d->streams[s], d->entry[e], 0));
  }
  c->in_dist = true;
  const bool self_p2p = emulated && getenv("PT_DIST_EMU_P2P") && atoi(getenv("PT_DIST_EMU_P2P")) == 1;
  // frames after the first of each kind (with and without an assembly) reuse
  // its launch parameters: nothing but the output and the assembled frame
  // change within a call (relaunch)
  Launched tmpl[2];
  for (int k = 0; k < n_frames && rc == PT_OK; ++k) {
    const int b = k % nsets;
    c->stream = d->streams[k % n_streams];
    Assembly as;
    if (k >= D) {
      const int pb = (k - D) % nsets;
      PT_HIP(hipStreamWaitEvent(c->stream, d->gather_done[pb], 0));
      if (d->rank == 0) {
        as.src = d->recv[pb];
        as.slot_floats = slot;
        as.frame = (float*)frames + (size_t)((k - D) % n_frame_bufs) * frame_f;
      }
    }
    float4* out = (float4*)(d->rank == 0 ? d->recv[b] : d->send[k % D]);
    Launched& t = tmpl[as.src ? 1 : 0];
    if (t.valid) {
      ptd::RenderParams p = t.p;
      p.pack_out = out;
      p.unpack_src = (const float4*)as.src;
      p.unpack_frame = (float4*)as.frame;
      if (as.src && dist_assembled(d, as.frame, c->unpack_key)) {   // live items only
        p.unpack_table = c->d_unpack_live;
        p.n_unpack = c->n_unpack_live;
      } else if (as.src) {
        p.unpack_table = c->d_unpack;
        p.n_unpack = c->n_unpack;
        dist_mark_assembled(d, as.frame, c->unpack_key);
      }
      rc = relaunch(c, p, t.lds, t.cnt);
    } else {
      rc = render_impl(c, 0, n_batches, out, as, &t);   // a whole assembly (the full table)
      if (rc == PT_OK && as.src) dist_mark_assembled(d, as.frame, c->unpack_key);
    }
    if (rc) break;
    PT_HIP(hipEventRecord(d->render_done[b], c->stream));
    PT_HIP(hipStreamWaitEvent(d->comm_stream, d->render_done[b], 0));
    if (emulated && self_p2p) {
      // measurement (PT_DIST_EMU_P2P=1): the other ranks' slots through
      // RCCL itself -- one grouped self send/recv per emulated rank, the
      // calls the root's real gather makes -- so the emulated step carries
      // RCCL's host and device cost per frame
      PT_NCCL(R->GroupStart());
      for (int r = 1; r < c->nranks; ++r) {
        PT_NCCL(R->Send(d->ingest + (size_t)(r - 1) * slot, slot, ncclFloat32, 0, d->comm, d->comm_stream));
        PT_NCCL(R->Recv(d->recv[b] + (size_t)r * slot, slot, ncclFloat32, 0, d->comm, d->comm_stream));
      }
      PT_NCCL(R->GroupEnd());
    } else if (emulated) {   // the other ranks' slots: the bytes a real gather would write here
      PT_HIP(hipMemcpyAsync(d->recv[b] + slot, d->ingest, (size_t)(c->nranks - 1) * slot * sizeof(float),
                            hipMemcpyDeviceToDevice, d->comm_stream));
    }
    if (d->nranks > 1) {
      PT_NCCL(R->GroupStart());
      if (d->rank == 0)
        for (int r = 1; r < d->nranks; ++r)
          PT_NCCL(R->Recv(d->recv[b] + (size_t)r * slot, slot, ncclFloat32, r, d->comm, d->comm_stream));
      else
        PT_NCCL(R->Send(d->send[k % D], slot, ncclFloat32, 0, d->comm, d->comm_stream));
      PT_NCCL(R->GroupEnd());
    }
    PT_HIP(hipEventRecord(d->gather_done[b], d->comm_stream));
  }
  c->in_dist = false;
  // the root assembles the last (up to) D frames in launches of their own
  if (rc == PT_OK && d->rank == 0) {
    frame_key(c, c->last, &c->key_scratch);
    rc = unpack_table(c, c->last, c->key_scratch);
    for (int k = std::max(0, n_frames - D); k < n_frames && rc == PT_OK; ++k) {
      const int b = k % nsets;
      c->stream = d->streams[k % n_streams];
      PT_HIP(hipStreamWaitEvent(c->stream, d->gather_done[b], 0));
      float4* out = (float4*)((float*)frames + (size_t)(k % n_frame_bufs) * frame_f);
      const bool live_only = dist_assembled(d, out, c->unpack_key);
      PT_HIP(ptd::launch_items_unpack(c->last, out, (const float4*)d->recv[b], slot / 4,
                                      live_only ? c->d_unpack_live : c->d_unpack,
                                      live_only ? c->n_unpack_live : c->n_unpack, c->stream));
      if (!live_only) dist_mark_assembled(d, out, c->unpack_key);
    }
  }
  // one use event per stream for the whole run (the launches above skip theirs)
  for (int sidx = 0; sidx < n_streams && rc == PT_OK; ++sidx) {
    c->stream = d->streams[sidx];
    rc = note_use(c);
  }
  c->stream = saved;
  return rc;
}

int pt_dist_set_streams(pt_context* c, void* render0, void* render1, void* comm) {
  PT_SINGLE(c, "pt_dist_set_streams");
  if (!c || !c->dist) return fail(PT_ERR_INVALID, "pt_dist_set_streams: no communicator (pt_dist_init)");
  DistState* d = c->dist;
  PT_HIP(hipSetDevice(c->device));
  for (hipStream_t s : {d->streams[0], d->streams[1], d->streams[2], d->comm_stream}) PT_HIP(hipStreamSynchronize(s));
  d->streams[0] = render0 ? (hipStream_t)render0 : d->own[0];
  d->streams[1] = render1 ? (hipStream_t)render1 : d->own[1];
  d->caller_streams = render0 || render1;
  d->comm_stream = comm ? (hipStream_t)comm : d->own[kDistStreams];
  return PT_OK;
}

int pt_dist_slot_floats(pt_context* c, size_t* slot_floats) {
  PT_SINGLE(c, "pt_dist_slot_floats");
  if (!c || !slot_floats) return fail(PT_ERR_INVALID, "null argument");
  if (!c->dist || !c->dist->slot_floats) return fail(PT_ERR_INVALID, "no pt_dist_run yet");
  *slot_floats = c->dist->slot_floats;
  return PT_OK;
}

int pt_dist_wait(pt_context* c, int timeout_ms) {
  PT_SINGLE(c, "pt_dist_wait");
  if (!c || !c->dist) return fail(PT_ERR_INVALID, "pt_dist_wait: no communicator");
  DistState* d = c->dist;
  PT_HIP(hipSetDevice(c->device));
  const auto t0 = std::chrono::steady_clock::now();
  for (;;) {
    bool done = true;
    for (hipStream_t s : {d->streams[0], d->streams[1], d->streams[2], d->comm_stream}) {
      const hipError_t q = hipStreamQuery(s);
      if (q == hipErrorNotReady) done = false;
      else if (q != hipSuccess) return fail(PT_ERR_HIP, std::string("pt_dist_wait: ") + hipGetErrorString(q));
    }
    if (done) return PT_OK;
    const long long ms = std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t0).count();
    if (timeout_ms >= 0 && ms > timeout_ms) return fail(PT_ERR_HIP, "pt_dist_wait: timed out (gather not complete)");
    std::this_thread::sleep_for(std::chrono::microseconds(200));
  }
}

int pt_dist_abort(pt_context* c) {
  PT_SINGLE(c, "pt_dist_abort");
  if (!c || !c->dist) return PT_OK;
  const RcclApi* R = rccl_api();
  if (c->dist->comm && R) (void)R->CommAbort(c->dist->comm);   // ends outstanding transfers
  c->dist->comm = nullptr;
  return pt_dist_finalize(c);
}

int pt_dist_finalize(pt_context* c) {
  if (!c) return fail(PT_ERR_INVALID, "null context");
  DistState* d = c->dist;
  if (!d) return PT_OK;
  (void)hipSetDevice(c->device);
  for (hipStream_t s : {d->streams[0], d->streams[1], d->streams[2], d->comm_stream})
    if (s) (void)hipStreamSynchronize(s);
  const RcclApi* R = rccl_api();
  if (d->comm && R) (void)R->CommDestroy(d->comm);
  dev_free(d->ingest);
  for (int b = 0; b < kDistStreams; ++b) dev_free(d->send[b]);
  for (hipStream_t s : d->own)
    if (s) (void)hipStreamDestroy(s);
  for (int b = 0; b < kDistSets; ++b) {
    dev_free(d->recv[b]);
    if (d->render_done[b]) (void)hipEventDestroy(d->render_done[b]);
    if (d->gather_done[b]) (void)hipEventDestroy(d->gather_done[b]);
  }
  for (hipEvent_t e : d->entry)
    if (e) (void)hipEventDestroy(e);
  delete d;
  c->dist = nullptr;
  return PT_OK;
}

}  // extern "C"
