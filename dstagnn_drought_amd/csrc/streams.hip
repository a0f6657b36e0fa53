// streams.hip — the side stream and the fork / join dependencies of the block (streams.hpp).
#include "streams.hpp"

#include <cstring>
#include <mutex>
#include <vector>

namespace {

__global__ void debug_delay_kernel(uint64_t ticks) {
  const uint64_t t0 = wall_clock64();
  while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
}

// DSTAGNN_DEBUG_STREAMS=1: the fork invariant check (Streams::side)
bool stream_debug() {
  static const bool on = env_flag("DSTAGNN_DEBUG_STREAMS", false);
  return on;
}

int fail(hipError_t r) {
  set_last_error(std::string("side stream: ") + hipGetErrorString(r));
  return (int)r;
}

}  // namespace

int debug_delay(hipStream_t q, bool on_main) {
  static const int us_main = env_int("DSTAGNN_DEBUG_MAIN_DELAY_US", 0);
  static const int us_side = env_int("DSTAGNN_DEBUG_SIDE_DELAY_US", 0);
  const int us = std::min(on_main ? us_main : us_side, 20000);
  if (us <= 0) return 0;
  static const int rate_khz = [] {
    int dev = 0, r = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&r, hipDeviceAttributeWallClockRate, dev) != hipSuccess)
      r = 0;
    return r > 0 ? r : 100000;
  }();
  hipLaunchKernelGGL(debug_delay_kernel, dim3(1), dim3(64), 0, q, (uint64_t)us * (uint64_t)rate_khz / 1000u);
  DS_CHECK_LAUNCH();
  return 0;
}

SideStream* side_stream_for_device() {
  static std::mutex mu;
  static SideStream cache[64];
  static const bool enabled = env_flag("DSTAGNN_SIDE_STREAM", true);
  if (!enabled) return nullptr;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
  std::lock_guard<std::mutex> lock(mu);
  SideStream& s = cache[dev];
  if (!s.ok) {
    int lo = 0, hi = 0;
    if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) lo = 0;
    // DSTAGNN_SIDE_CUMASK=0x<32-bit pattern>: the side stream confined to the CUs the pattern
    // selects (replicated over every 32-CU word; A/B knob: the side stream's weight-gradient
    // GEMMs otherwise take CUs from the latency-bound main chain); no priority with a mask
    // (hipExtStreamCreateWithCUMask takes no flags: that stream is BLOCKING, so with a caller on
    // the legacy null stream it also serialises with it — measurements under this knob include
    // that serialisation)
    static const char* const cm = env_str("DSTAGNN_SIDE_CUMASK");
    if (cm && *cm) {
      const uint32_t pat = (uint32_t)strtoul(cm, nullptr, 0);
      int ncu = 0;
      if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || ncu <= 0) ncu = 256;
      std::vector<uint32_t> mask((size_t)(ncu + 31) / 32, pat);  // one 32-bit word per 32 CUs
      if (ncu % 32) mask.back() &= (1u << (ncu % 32)) - 1u;
      if (hipExtStreamCreateWithCUMask(&s.side, (uint32_t)mask.size(), mask.data()) != hipSuccess) return nullptr;
    } else if (hipStreamCreateWithPriority(&s.side, hipStreamNonBlocking, lo) != hipSuccess) {
      return nullptr;
    }
    for (auto& e : s.ev)
      if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return nullptr;
    s.ksig = env_flag("DSTAGNN_KSIG", true);
    if (hipMalloc(&s.flags, sizeof(uint32_t) * SideStream::kSlots) != hipSuccess ||
        hipMemset(s.flags, 0, sizeof(uint32_t) * SideStream::kSlots) != hipSuccess ||
        hipDeviceSynchronize() != hipSuccess)
      return nullptr;
    s.ok = true;
  }
  return &s;
}

void Streams::init(hipStream_t main) {
  st = main;
  ss = gemm_prof_on() ? nullptr : side_stream_for_device();
  sd = ss ? ss->side : st;
}

hipStream_t Streams::side() {
  if (stream_debug() && open_forks > 0 && !order_err) {
    set_last_error("stream invariant: side-stream work issued before its fork's signal went out");
    order_err = DSTAGNN_E_ARG;
  }
  return sd;
}

ForkSig Streams::claim_sig() {
  ForkSig sig;
  sig.p = ss->flags + ss->fnext.fetch_add(1, std::memory_order_relaxed) % SideStream::kSlots;
  sig.v = ss->gseq.fetch_add(1, std::memory_order_relaxed) + 1;
  return sig;
}

int Streams::send_sig(const ForkSig& sig) {
  hipError_t r = sig.carried ? hipSuccess : hipStreamWriteValue32(st, sig.p, sig.v, 0);
  // the writer is queued: now the side's wait
  if (r == hipSuccess) r = hipStreamWaitValue32(sd, sig.p, sig.v, hipStreamWaitValueGte, 0xffffffffu);
  return r == hipSuccess ? debug_delay(sd, false) : fail(r);
}

int Streams::signal(hipStream_t from, SyncTok* t) {
  *t = SyncTok{};
  if (!ss) return 0;
  if (from != ss->side) {  // made by the main stream: a flag write
    const ForkSig sig = claim_sig();
    t->slot = (int)(sig.p - ss->flags);
    t->seq = sig.v;
    const hipError_t r = hipStreamWriteValue32(from, sig.p, sig.v, 0);
    return r == hipSuccess ? 0 : fail(r);
  }
  t->ev = ss->ev[ss->next.fetch_add(1, std::memory_order_relaxed) % 64];  // by the side stream: an event
  const hipError_t r = hipEventRecord(t->ev, from);
  return r == hipSuccess ? 0 : fail(r);
}

int Streams::wait(hipStream_t to, const SyncTok& t) {
  if (to == st && open_forks > 0) {  // the side's wait for the open fork is not queued: both would wait
    set_last_error("stream invariant: the main stream waits for the side stream inside a fork_on scope");
    return DSTAGNN_E_ARG;
  }
  hipError_t r = hipSuccess;
  if (t.slot >= 0)
    r = hipStreamWaitValue32(to, ss->flags + t.slot, t.seq, hipStreamWaitValueGte, 0xffffffffu);
  else if (t.ev)
    r = hipStreamWaitEvent(to, t.ev, 0);
  return r == hipSuccess ? 0 : fail(r);
}

static int event_pair(Streams& ks, hipStream_t from, hipStream_t to) {
  if (from == to) return 0;
  SyncTok t;
  DS_TRY(ks.signal(from, &t));
  return ks.wait(to, t);
}

int Streams::fork() {
  DS_TRY(event_pair(*this, st, sd));
  return split() ? debug_delay(sd, false) : 0;
}

int Streams::join() { return event_pair(*this, sd, st); }
