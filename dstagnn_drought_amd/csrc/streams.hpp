// streams.hpp — the block's two streams: the caller's (main) stream, the per-device side
// stream, and the dependencies between them (streams.hip).
#pragma once
#include <atomic>

#include "common.hpp"

// The backward has two dependency chains: the data gradients (dx -> ... -> d_x, each step
// needing the previous) and the parameter gradients (weight GEMMs, bias / gamma / beta
// column sums, split-K folds), which only read values the data chain has produced. The
// second chain runs on a side stream (lowest priority) forked from the caller's stream
// by events, so its kernels fill the CUs the small data-chain kernels leave idle; it has
// its own GEMM / reduction workspaces and its inputs are never overwritten by the main
// chain afterwards (buffers that would be are given their own allocation). One join at
// the end. DSTAGNN_SIDE_STREAM=0 runs everything on the caller's stream.
struct SideStream {
  hipStream_t side = nullptr;
  hipEvent_t ev[64] = {};
  // ring positions and sequence numbers are claimed atomically: the SideStream is shared by
  // every caller on the device (e.g. the autograd device thread and a forward on another
  // thread), and two callers must never get the same slot or sequence number
  std::atomic<uint32_t> next{0};
  // flag words for stream-ordered write / wait-value synchronisation (see Streams)
  static constexpr int kSlots = 4096;  // divides 2^32: the claimed counters wrap consistently
  uint32_t* flags = nullptr;
  std::atomic<uint32_t> gseq{0};
  std::atomic<uint32_t> fnext{0};
  bool ksig = true;         // fork_on flags written by the kernel the caller names (DSTAGNN_KSIG=0: off)
  bool ok = false;
};
SideStream* side_stream_for_device();  // null when disabled (DSTAGNN_SIDE_STREAM=0) or unavailable

// Race probes (tests/test_gpu_knobs.py): DSTAGNN_DEBUG_MAIN_DELAY_US / DSTAGNN_DEBUG_SIDE_DELAY_US
// put a bounded busy-wait kernel (<= 20 ms, one wave) on the main stream before every stage /
// on the side stream after every fork, so a cross-stream read issued without its dependency
// reads stale data instead of winning the race by timing (a missing fork once went unnoticed
// because the side stream happened to reach the read late).
int debug_delay(hipStream_t q, bool on_main);

// One cross-stream dependency: the consumer stream's later work waits for everything the
// producer stream had issued when the token was made.
struct SyncTok {
  hipEvent_t ev = nullptr;
  int slot = -1;
  uint32_t seq = 0;
};

// fork / join between the caller's stream and the side stream (no-ops when disabled).
// Prices on gfx950 / ROCm 7.2 (tools/fork_probe.hip, tools/flag_sync_probe.hip, step timelines):
// an hipEventRecord between two kernels idles the RECORDING stream ~5.6 us, while waiting for an
// event that has already completed costs the waiting stream nothing; a stream-ordered flag write
// (hipStreamWriteValue32 of a fresh sequence number into a device-memory flag word, after all
// prior work of the producer stream) and a flag wait (hipStreamWaitValue32, >= that number) run
// as small ROCclr kernels of ~4 us each on their streams.  (Flags in hipMallocSignalMemory do
// NOT order the data: stale reads in flag_sync_probe; device memory: 0 stale reads in 600
// rounds both ways.)  So the main chain never records an event: a dependency made BY the main
// stream (fork) is a flag write on main + a flag wait on the side; one made by the side stream
// (join, dx_ready) is an event recorded on the side, usually complete by the time the main
// stream waits for it.  Flag words rotate over kSlots; numbers only grow, so a wait can only
// be released by its own write or a later one issued behind it.
// Kernel-written fork flags (fork_on; default, DSTAGNN_KSIG=0 for the hipStreamWriteValue32
// above): the flag is stored by workgroup 0 of the main-stream launch the caller hands to
// fork_on (a carrier, common.hpp) — every earlier kernel of the stream has completed when it
// starts — and the side's wait is queued when that launch has returned, before the side's work:
// the writer always precedes the wait in host order (a first version queued the wait at the
// fork and hung with a CU-masked side stream).  tools/flag_sync_probe.hip modes 4 / 5: 0 stale
// reads in 300 rounds each way.
// This relies on the HIP runtime setting the AQL barrier bit on every same-stream dispatch (a
// kernel's workgroup 0 starts only once every earlier kernel of the stream has completed; true
// for ROCm 7.2's in-order streams).  Nothing checks it at run time: after a runtime upgrade run
// the race probes (tests/test_gpu_knobs.py, DSTAGNN_DEBUG_*_DELAY_US with the default
// DSTAGNN_KSIG=1; tools/gpu_check.sh knobs) before trusting the flags; DSTAGNN_KSIG=0 falls
// back to hipStreamWriteValue32.
// Invariant: no side-stream work is issued, and the main stream never waits for the side,
// inside a fork_on scope — the scope's side wait is not queued yet.  The first is recorded by
// side() under DSTAGNN_DEBUG_STREAMS=1 (order_err, returned at the next stage boundary); the
// second would deadlock and is always an error (wait / join).
struct Streams {
  hipStream_t st = nullptr, sd = nullptr;  // sd == st when the side stream is off
  SideStream* ss = nullptr;
  int open_forks = 0;  // fork_on scopes whose launch is running
  int order_err = 0;
  void init(hipStream_t main);
  bool split() const { return sd != st; }
  hipStream_t side();  // the side stream, for a launch
  int signal(hipStream_t from, SyncTok* t);
  int wait(hipStream_t to, const SyncTok& t);
  int fork();  // side sees everything the main chain issued so far
  int join();  // main waits for everything issued on the side
  // fork() whose flag rides on a main-stream launch the caller names: int launch(ForkSig*),
  // which passes the signal to ONE carrier (null: nothing to carry).  A signal the launch did
  // not carry (e.g. a skinny GEMM took it) is written on main here.  The side work that
  // depends on the fork follows the call.
  template <class Launch>
  int fork_on(Launch&& launch) {
    if (!(ss && ss->ksig && split())) {
      DS_TRY(fork());
      return launch(nullptr);
    }
    ForkSig sig = claim_sig();
    ++open_forks;
    const int r = launch(&sig);
    --open_forks;
    return r ? r : send_sig(sig);  // (a failed launch: nothing is pending)
  }

 private:
  ForkSig claim_sig();
  int send_sig(const ForkSig& sig);  // the write unless carried, the side's wait, the side delay
};
