// Host half shared by the device epoch runners (skge_epoch.hip,
// skge_pipeline.hip, skge_pairloop.hip, skge_tripleloop.hip): the batch
// geometry, the argument refusals, and GraphRunnerCore -- the captured graph
// and the device buffers it names.  A runner supplies its own checks beyond
// check_runner_args, its buffers (alloc) and the launches between
// begin_capture and end_capture; the pair and triple loops' creates share
// more than that, and are written on skge_loop_runner.h.
#pragma once
#include <cstdint>
#include <memory>
#include <utility>
#include <vector>

#include "skge_epoch_batches.h"
#include "skge_host.h"

namespace skge {

// set the error text; converts to any runner's NULL handle
template <class... A>
inline std::nullptr_t fail(const char* fmt, A... a) {
  if constexpr (sizeof...(A) == 0) set_error("%s", fmt);
  else set_error(fmt, a...);
  return nullptr;
}

// The refusals every runner makes before its first HIP call.  Tmax and cap_min
// are the runner's own bounds: the pair loop indexes 2T pairs with ints and the
// triple loop 3T triples; the pair and triple loops and the device sampler
// need a set of >= 2T slots, the pipelined runner takes any set of >= 4.
inline bool check_runner_args(const char* who, const void* trip, const void* set,
                              const void* epoch_key, int64_t T, int64_t Tmax, int nbatches,
                              int64_t set_capacity, int64_t cap_min, int ntries, void* stream) {
  auto no = [who](const char* fmt, long long bound) {
    char what[96];
    snprintf(what, sizeof(what), fmt, bound);
    set_error("%s: %s", who, what);
    return false;
  };
  if (!trip || !set || !epoch_key) return no("NULL argument", 0);
  if (T <= 0 || T > Tmax)
    return Tmax == INT64_MAX ? no("T must be >= 1", 0) : no("T must be in [1, %lld]", Tmax);
  if (nbatches < 1 || nbatches > T) return no("nbatches must be in [1, T]", 0);
  if (set_capacity < cap_min || (set_capacity & (set_capacity - 1)))
    return no("set capacity must be a power of 2 >= %lld", cap_min);
  if (ntries < 1) return no("ntries >= 1", 0);
  if (!stream) return no("needs a non-default stream (graph capture)", 0);
  return true;
}

// One captured epoch and the device buffers its nodes name.  Runner structs
// derive from it; deleting a runner releases everything.
struct GraphRunnerCore {
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  int nnodes = 0;             // nodes of the captured graph
  std::vector<void*> bufs;
  bool alloc_ok = true;       // false once an alloc() has failed
  size_t alloc_bytes = 0;     // bytes alloc() was asked for so far

  GraphRunnerCore() = default;
  GraphRunnerCore(const GraphRunnerCore&) = delete;
  GraphRunnerCore& operator=(const GraphRunnerCore&) = delete;

  // A device buffer owned by the runner.  zero: at least 4 bytes, zero-filled
  // before this returns; otherwise as hipMalloc leaves it (the graph writes it
  // before it reads it).  nullptr on failure (alloc_ok stays false).
  void* alloc(size_t bytes, bool zero) {
    if (zero && bytes < 4) bytes = 4;
    alloc_bytes += bytes;
    void* p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) {
      alloc_ok = false;
      return nullptr;
    }
    bufs.push_back(p);
    if (zero && hipMemset(p, 0, bytes) != hipSuccess) {
      alloc_ok = false;
      return nullptr;
    }
    return p;
  }

  // the stream's earlier work done (the caller's tables, the zero fills), then
  // thread-local capture
  bool begin_capture(hipStream_t st) {
    if (hipStreamSynchronize(st) == hipSuccess &&
        hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) == hipSuccess)
      return true;
    set_error("hipStreamBeginCapture failed");
    return false;
  }

  // rc: the captured launches' result (its error text already set).  Ends the
  // capture either way; on success the graph is instantiated and counted.
  bool end_capture(hipStream_t st, int rc) {
    hipError_t e = hipStreamEndCapture(st, &graph);
    if (!rc && e != hipSuccess) set_error("hipStreamEndCapture: %s", hipGetErrorString(e));
    if (rc || e != hipSuccess) {
      if (graph) (void)hipGraphDestroy(graph);
      graph = nullptr;
      return false;
    }
    size_t n = 0;
    if (hipGraphGetNodes(graph, nullptr, &n) == hipSuccess) nnodes = (int)n;
    e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    if (e != hipSuccess) set_error("hipGraphInstantiate: %s", hipGetErrorString(e));
    return e == hipSuccess;
  }

  hipError_t launch(hipStream_t st, int nepochs) {
    hipError_t e = hipSuccess;
    for (int i = 0; i < nepochs && e == hipSuccess; ++i) e = hipGraphLaunch(exec, st);
    return e;
  }

  ~GraphRunnerCore() {
    if (exec) (void)hipGraphExecDestroy(exec);
    if (graph) (void)hipGraphDestroy(graph);
    for (void* p : bufs) (void)hipFree(p);
    // HIP's last-error word is sticky.  A runner is deleted right after a
    // failed allocation or capture; the error is cleared here, once, after the
    // frees, so that it cannot fail a later launch check.
    (void)hipGetLastError();
  }
};

// the run / nlaunches bodies of the runners that are nothing but their graph
inline int run_graph(GraphRunnerCore* r, void* stream, int nepochs) {
  SKGE_CHECK_ARG(r && r->exec, "bad runner");
  SKGE_CHECK_HIP(r->launch(as_stream(stream), nepochs));
  return SKGE_OK;
}

// A run()'s ordering against the caller's stream (skge_run_order_begin / _end,
// include/skge_hip.h; one implementation for every runner family), paid for
// on the host: by default neither stream receives a cross-stream event wait.
//
// begin: the caller's earlier work done before the runner's first launch.
// 0: nothing in flight on the caller's stream (or one stream), nothing
// enqueued anywhere; 1: the host waited for the caller's stream.
inline int run_order_begin(void* run_stream, void* caller_stream) {
  SKGE_CHECK_ARG(run_stream, "run_order_begin: needs the runner's (non-default) stream");
  if (run_stream == caller_stream) return 0;
  const hipError_t e = hipStreamQuery(as_stream(caller_stream));
  if (e == hipSuccess) return 0;
  // (a not-ready answer must not stay behind as HIP's last error: the launch
  // checks read that word)
  (void)hipGetLastError();
  if (e != hipErrorNotReady) {
    set_error("run_order_begin: hipStreamQuery(caller_stream): %s", hipGetErrorString(e));
    return SKGE_EHIP;
  }
  SKGE_CHECK_HIP(hipStreamSynchronize(as_stream(caller_stream)));
  return 1;
}

// end: the caller's later work after the runner's launches.  0: one stream,
// nothing to do.  1 (queued == 0): the host waited for the runner's stream --
// the wait queued on the caller's stream is what slows the replays down (the
// other hardware queue holds an unsatisfied barrier while they run; measured,
// profiles/run_ordering), so by default none is queued.  2 (queued != 0): an
// event recorded on the runner's stream (no timing), waited for by the
// caller's, released at once (the runtime keeps it until it fires).
inline int run_order_end(void* run_stream, void* caller_stream, int queued) {
  SKGE_CHECK_ARG(run_stream, "run_order_end: needs the runner's (non-default) stream");
  if (run_stream == caller_stream) return 0;
  if (!queued) {
    SKGE_CHECK_HIP(hipStreamSynchronize(as_stream(run_stream)));
    return 1;
  }
  hipEvent_t ev = nullptr;
  SKGE_CHECK_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  hipError_t e = hipEventRecord(ev, as_stream(run_stream));
  if (e == hipSuccess) e = hipStreamWaitEvent(as_stream(caller_stream), ev, 0);
  const hipError_t d = hipEventDestroy(ev);
  SKGE_CHECK_HIP(e);
  SKGE_CHECK_HIP(d);
  return 2;
}

}  // namespace skge
