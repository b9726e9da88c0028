// diag.h — what a diagnostic build of the kernels is, stated once.  Three build switches
// (build.py: HFG_EXTRA_FLAGS=-D<switch>=1), all 0 in the shipped library, whose device code
// holds none of this:
//   HFG_ABLATE       kernel ablations for timing experiments, chosen at run time by the bits of
//                    the DEBUG_FLAGS schedule knob (hfg_debug_schedule_set; bench.py --sched)
//   HFG_CONV_TIMING  clock stamps of the tile-5 layer-conv kernel (conv_bf16x3.hip)
//   HFG_RB_TIMING    clock stamps of the whole-ResBlock kernels (resblock_body.h)
// Included by kernels.h, so every kernel unit and the host orchestration see the same values.
#pragma once

#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>

#ifndef HFG_ABLATE
#define HFG_ABLATE 0
#endif
#ifndef HFG_CONV_TIMING
#define HFG_CONV_TIMING 0
#endif
#ifndef HFG_RB_TIMING
#define HFG_RB_TIMING 0
#endif

namespace hfg {

// ---- ablations (the `dbg` field of ConvParams, UpsParams and RbParams) ----
// A use site reads `kAblate && (dbg & kAbl...)`: false at compile time in the shipped build.
// One knob drives every kernel, so the bits are disjoint (asserted below).  An ablated run
// times a kernel with one piece of its work removed; "wrong": its results are.
constexpr bool kAblate = HFG_ABLATE != 0;
enum AblateBit : int {
  // conv1d_bf16x3 (conv_bf16x3.hip)
  kAblConvNoRestage = 1,     // runtime-tap loop: no input staging after the first group; wrong
  kAblConvNoBarrier = 4,     // no per-chunk / per-group barrier; racy, wrong
  kAblConvNoEpilogue = 8,    // returns after the main loop; nothing stored, wrong
  kAblConvWarmX = 128,       // every group's input loads re-read channel group 0 (L2-warm); wrong
  kAblConvUpsRawX = 256,     // polyphase upsampler: raw fp32 halves staged, no lrelu / split; wrong
  kAblConvNoLoB = 4096,      // AREG tiles: no lo-plane LDS reads (the hi fragment stands in); wrong
  // conv_epilogue_lds2 (epilogue.h), the AREG tiles' epilogue
  kAblEpiNoStore = 16384,    // interior tiles: no output stores; wrong
  kAblEpiWarmRes = 32768,    // residual read from row 0's columns (L2-warm); wrong
  kAblEpiNoRes = 65536,      // residual not read (taken as 0); wrong
  // resblock_bf16x3 / resblock2_bf16x3 (resblock_body.h)
  kAblRbNoMrf = 16,          // no MRF epilogue (no read-modify-write); nothing stored, wrong
  kAblRbZeroX = 32,          // x zeroed after its loads; wrong
  kAblRbNoOperand = 64,      // no operand writes to LDS; wrong
  kAblRbNoLoB = 2048,        // no lo-plane LDS reads (the hi fragment stands in); wrong
  // ups_bf16x3 (ups_bf16x3.hip)
  kAblUpsNoStoreX = 512,     // no input conversion / LDS store after group 0; wrong
  kAblUpsNoLoadX = 1024,     // no input loads after group 0; wrong
  kAblUpsSlab0 = 131072,     // no weight slab after group 0's (every group re-reads it); wrong
  kAblUpsNoStoreY = 262144,  // no output stores; wrong
};
constexpr int kAblateBits[] = {
    kAblConvNoRestage, kAblConvNoBarrier, kAblConvNoEpilogue, kAblConvWarmX, kAblConvUpsRawX,
    kAblConvNoLoB,     kAblEpiNoStore,    kAblEpiWarmRes,     kAblEpiNoRes,  kAblRbNoMrf,
    kAblRbZeroX,       kAblRbNoOperand,   kAblRbNoLoB,        kAblUpsNoStoreX, kAblUpsNoLoadX,
    kAblUpsSlab0,      kAblUpsNoStoreY};
constexpr bool ablate_bits_disjoint() {
  int seen = 0;
  for (int b : kAblateBits) {
    if (b <= 0 || (b & (b - 1)) || (seen & b)) return false;
    seen |= b;
  }
  return true;
}
static_assert(ablate_bits_disjoint(), "every ablation is one bit of DEBUG_FLAGS, none shared");

// ---- clock stamps ----
// Wave 0 of a block stamps the shader clock (s_memtime) at its phase boundaries and the 100 MHz
// clock (s_memrealtime) at its start and end, and stores the slots once at its end into
// [regions][blocks][slots] uint64 in device memory: a store in mid-kernel would make every
// later vmcnt wait also wait for its write.  Read back by hfg_debug_{cv,rb}_ts, whose shape
// hfg_debug_{cv,rb}_ts_geometry reports (tests/tools/conv_phases.py, rb_phases.py).
struct TsGeometry {
  int slots, blocks, regions;
  constexpr size_t words() const { return (size_t)regions * blocks * slots; }
};
// conv1d_bf16x3, tiles 5 and 6: region = (taps 3, 7, 11, other) x (plain, residual,
// residual + MRF add); block = linear block index modulo blocks
constexpr TsGeometry kCvTs = {16, 8192, 12};
enum CvTsSlot : int {
  kCvTsStart = 0,      // realtime
  kCvTsSetup = 1,      // clock: setup done, the prologue begins
  kCvTsPrologue = 2,   // prologue done
  kCvTsLoop = 3,       // channel-group loop done
  kCvTsEnd = 4,        // epilogue done
  kCvTsBarWait = 5,    // cycles: the loop's summed barrier waits (not a stamp)
  kCvTsEndReal = 6,    // realtime
  kCvTsEpiBarrier = 7, // the epilogue's barrier passed
  kCvTsEpiTile = 8,    // + 2i: row tile i staged in LDS, + 2i + 1: its stores issued (i < 2)
  kCvTsHwId = 12,      // HW_ID | XCC_ID << 32 of the wave (not a stamp)
};
// resblock_bf16x3 / resblock2_bf16x3: region = (k 3, 7, 11) x (C 32, 64, 128) x launch half,
// then the narrow C = 64 window's two halves; block = linear block index (past blocks: block 0).
// The stamps live in LDS until the end: RbLds::ts_bytes (lds_layout.h).
constexpr TsGeometry kRbTs = {24, 8192, 20};
enum RbTsSlot : int {
  kRbTsStart = 0,     // realtime
  kRbTsSetup = 1,     // clock: the window is chosen
  kRbTsPrologue = 2,  // the first operand is in LDS
  kRbTsConv = 3,      // + 2cv: conv cv's MFMA loop done; + 2 n_conv: the MRF epilogue done
  kRbTsTrans = 4,     // + 2cv: conv cv's result is the next operand; + 2 n_conv: realtime end
  kRbTsSub = 20,      // the first of the sub-phase stamps; the slots below it are the sequence
  kRbTsLoadsIssued = 20,  // A-stream loads issued
  kRbTsXLanded = 21,      // f16x3: x has landed
  kRbTsAmax = 22,         // f16x3: the block's exponent is known
  kRbTsMrfLanded = 23,    // the MRF values have landed
};
static_assert(kCvTsHwId < kCvTs.slots && kRbTsMrfLanded < kRbTs.slots, "slots inside a block's row");

// ---- readback of a stamp buffer (diagnostic builds; host) ----
inline int ts_read(const void* symbol, size_t size, void* dst, size_t bytes) {
  return (int)hipMemcpyFromSymbol(dst, symbol, bytes < size ? bytes : size, 0,
                                  hipMemcpyDeviceToHost);
}
inline int ts_clear(const void* symbol, size_t size) {
  void* dev = nullptr;
  hipError_t e = hipGetSymbolAddress(&dev, symbol);
  if (e == hipSuccess) e = hipMemset(dev, 0, size);
  return (int)e;
}
// The C entries of one stamp buffer.  They exist only in that diagnostic build, so they are
// not declared in include/ (the Python loader refuses a library that lacks a declared symbol).
#define HFG_TS_ENTRIES(tag, buffer, geometry)                                          \
  extern "C" int hfg_debug_##tag##_ts(void* dst, size_t bytes) {                       \
    return hfg::ts_read(&buffer, sizeof(buffer), dst, bytes);                          \
  }                                                                                    \
  extern "C" int hfg_debug_##tag##_ts_clear() {                                        \
    return hfg::ts_clear(&buffer, sizeof(buffer));                                     \
  }                                                                                    \
  extern "C" void hfg_debug_##tag##_ts_geometry(int* slots, int* blocks, int* regions) { \
    *slots = geometry.slots, *blocks = geometry.blocks, *regions = geometry.regions;   \
  }

}  // namespace hfg
