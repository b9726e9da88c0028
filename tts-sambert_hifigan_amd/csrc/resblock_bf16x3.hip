// resblock_bf16x3.hip — one whole ResBlock per launch (bf16x3 MFMA), for the
// narrow stages (C in {32, 64}) where a layer-per-launch schedule is bound by HBM
// round trips, not by the matrix cores:
//
//   for m in dilations:  x = x + conv2_m(lrelu(conv1_m(lrelu(x))))   models/hifigan.py:79-85
//   mrf = (mrf + x) [/ n_res]                                         models/hifigan.py:125-131
//
// A block owns a window of NWIN time columns [ws, ws + NWIN) of one utterance and
// writes the centre [ws + halo, ws + halo + W), W = NWIN - 2*halo, where halo is the
// receptive-field radius of the launch's convs after the first (sum of (k-1)/2 * dilation).
// All convs run on the whole window.  The first conv's operand also covers its radius on
// either side (the LDS margin rows, staged from x), so its output is exact on the whole
// window; from the second conv on, the columns within a conv's radius of the window edge
// become garbage and the garbage front moves inwards by exactly that radius, so the
// centre is exact.  Columns outside [0, len) are re-zeroed after every conv — the
// reference's zero padding of each conv input.
//
// State: the residual stream x lives in registers (fp32, MFMA accumulator layout:
// every wave owns 32 rows x 128 columns of the window for the whole block), the
// current conv's B operand lives in LDS as bf16 hi/lo planes [group][plane][col][16]
// (one buffer, rewritten in place after a barrier).  The A operand (weights) is
// streamed from global memory (L2/L1-resident: every block reads the same stream)
// straight into registers two k-steps ahead; it is packed per wave row-block (rb_pack,
// pack_layout.h) so each k-step is 2 x 1 KB coalesced.
//
// Channel order inside a 16-channel group is permuted (slot 8h+e <-> channel
// 4h + (e&3) + 8(e>>2)) so that the rows one lane holds in the accumulator layout are
// exactly the 8 slots it reads as a B fragment: the epilogue writes the next conv's
// operand with one ds_write_b128 per plane and group.  The weight packer applies the
// same permutation to the K index.
//
// HBM traffic per ResBlock: x once (+ halo), MRF read-modify-write once, vs 5 tensor
// passes per dilation for the layer-per-launch schedule.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>
#include <mutex>

#include <cstdio>

#include "bf16x3_common.h"
#include "kernels.h"
#include "launch.h"

namespace hfg {

#if HFG_RB_TIMING
__device__ uint64_t g_rb_ts[kRbTs.words()];  // the clock stamps of these kernels (diag.h)
#endif

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// conv_post + tanh (models/hifigan.py:254-256) fused into the network's last MRF write (C = 32,
// one 32-row wave per window slice): the exact final x on the window columns [halo - 3,
// halo + W + 3) is staged as lrelu(x) in LDS ([channel][column + sh] fp32, 0 outside those
// columns and outside [0, len)), then one thread per 2 consecutive samples (each quad split over
// the two halves of the block) sums over (channel, tap) in conv_post4_tanh's order (channel-
// major, fma from 0, bias last): bitwise the separate kernel's wav, without the stage output's
// HBM write and read.
template <int NT, int NWIN, int WN>
__device__ __forceinline__ void conv_post_tail(const RbParams& p, const floatx16 (&xcur)[1][WN],
                                               const bool (&ok)[WN], char* lds, int b, int len_b,
                                               int t0, int tid, int cbase, int half, int col) {
  constexpr int C = 32, KP = 7;
  constexpr int S = rb_lds(C, NWIN).post_row;  // row stride (floats)
  typedef float f4 __attribute__((ext_vector_type(4)));
  float* const s = reinterpret_cast<float*>(lds);
  const int sh = (4 - (p.halo & 3)) & 3;  // staged column = window column + sh: 16-B aligned quads
  lds_barrier();                          // every wave is done reading the last conv's operand
  const float slope = p.post_slope;       // 0.1 (reference) or the handle's (release: 0.01)
#pragma unroll
  for (int k = 0; k < WN; ++k)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float v = xcur[0][k][r];
      s[acc_row(r, half) * S + cbase + 32 * k + col + sh] =
          ok[k] ? (v > 0.f ? v : v * slope) : 0.f;
    }
  lds_barrier();
  const float bias = p.post_b[0];
  float* const wav = p.wav + (int64_t)b * p.L;
  // the first half of the threads computes samples 0, 1 of each quad, the second half samples
  // 2, 3 (wave-uniform: two specialised code paths), so every wave works on the tail
  static_assert(NT % 128 == 0, "whole waves per half");
  const int hq = __builtin_amdgcn_readfirstlane(tid / (NT / 2));
  auto run = [&](auto h_tag) {
    constexpr int H = decltype(h_tag)::value;
    for (int q = tid - H * (NT / 2); q < p.W / 4; q += NT / 2) {
      const int t = t0 + 4 * q;  // p.L % 4 == 0 (host): a quad is wholly inside or past the row
      if (t >= p.L) break;
      // element k of v = column t - 4 + k (conv_post4_tanh's layout)
      const float* xs = s + p.halo + sh + 4 * q - 4;
      float acc[2] = {0.f, 0.f};
#pragma unroll 4
      for (int c = 0; c < C; ++c) {
        const f4 q0 = *reinterpret_cast<const f4*>(xs + c * S);
        const f4 q1 = *reinterpret_cast<const f4*>(xs + c * S + 4);
        const f4 q2 = *reinterpret_cast<const f4*>(xs + c * S + 8);
        const float v[12] = {q0[0], q0[1], q0[2], q0[3], q1[0], q1[1],
                             q1[2], q1[3], q2[0], q2[1], q2[2], q2[3]};
        const float* w = p.post_w + c * KP;
#pragma unroll
        for (int o = 0; o < 2; ++o)
#pragma unroll
          for (int j = 0; j < KP; ++j) acc[o] = fmaf(w[j], v[2 * H + o + j + 1], acc[o]);
      }
      floatx2_ r;
#pragma unroll
      for (int o = 0; o < 2; ++o) r[o] = t + 2 * H + o >= len_b ? 0.f : tanhf(acc[o] + bias);
      *reinterpret_cast<floatx2_*>(wav + t + 2 * H) = r;
    }
  };
  if (hq == 0)
    run(std::integral_constant<int, 0>{});
  else
    run(std::integral_constant<int, 1>{});
}

// both kernels are the text of resblock_body.h
#define HFG_RB2 0
#include "resblock_body.h"
#undef HFG_RB2
#define HFG_RB2 1
#include "resblock_body.h"
#undef HFG_RB2

namespace {

struct EntryRb {
  int kt, waves_m, waves_n, wm, np, fmt;
  bool persist;
  Instance<RbParams> inst;
  int C() const { return 32 * wm * waves_m; }
  int nwin() const { return 32 * (4 / wm) * waves_n; }
};

#define HFGRB_ENTRY(KT, WMS, WNS, WM, NP, FMT, PS) \
  { KT, WMS, WNS, WM, NP, FMT, PS, {resblock_bf16x3<KT, WMS, WNS, WM, NP, FMT, PS>, {0}} }
#define HFGRB_KTS(WMS, WNS, WM, NP, FMT, PS)                                                 \
  HFGRB_ENTRY(3, WMS, WNS, WM, NP, FMT, PS), HFGRB_ENTRY(5, WMS, WNS, WM, NP, FMT, PS),      \
      HFGRB_ENTRY(7, WMS, WNS, WM, NP, FMT, PS), HFGRB_ENTRY(11, WMS, WNS, WM, NP, FMT, PS)
// 32-row waves (WM 1): C = 64 (2 x 4 waves), C = 32 (1 x 4), C = 128 (4 x 2, k = 3),
// C = 64 narrow (2 x 2, k = 3).  64-row waves (WM 2: half the LDS operand reads per MFMA,
// twice the weight-fragment loads) measured the same in a same-box A/B (round 4) and are not
// instantiated.
// Persistent variants (PERSIST: a grid of resident blocks walks the windows, each window's
// x copied to LDS beside the previous window's MRF round trip) for C = 64 with the
// 512-column window (one block per CU).  Measured and not built: C = 128 (+0.9 %) and
// C = 32 (two blocks per CU: +2 to +5 %), profiles/r05/ab.
#define HFGRB_SET(NP, FMT)                                                                   \
  HFGRB_KTS(2, 4, 1, NP, FMT, false), HFGRB_KTS(1, 4, 1, NP, FMT, false),                     \
      HFGRB_ENTRY(3, 4, 2, 1, NP, FMT, false), HFGRB_ENTRY(3, 2, 2, 1, NP, FMT, false),        \
      HFGRB_KTS(2, 4, 1, NP, FMT, true)

// bf16x3 (NP 3, bf16), f16x3 (NP 3, f16), bf16w (NP 2 on the f16 kernels)
EntryRb g_entriesRb[] = {HFGRB_SET(3, 0), HFGRB_SET(3, 1), HFGRB_SET(2, 1)};

// ResBlock2 (resblock2_bf16x3): the same shapes per C, one window per block
#define HFGRB2_ENTRY(KT, WMS, WNS, WM, NP, FMT) \
  { KT, WMS, WNS, WM, NP, FMT, false, {resblock2_bf16x3<KT, WMS, WNS, WM, NP, FMT>, {0}} }
#define HFGRB2_KTS(WMS, WNS, WM, NP, FMT)                                       \
  HFGRB2_ENTRY(3, WMS, WNS, WM, NP, FMT), HFGRB2_ENTRY(5, WMS, WNS, WM, NP, FMT), \
      HFGRB2_ENTRY(7, WMS, WNS, WM, NP, FMT), HFGRB2_ENTRY(11, WMS, WNS, WM, NP, FMT)
#define HFGRB2_SET(NP, FMT)                                                      \
  HFGRB2_KTS(2, 4, 1, NP, FMT), HFGRB2_KTS(1, 4, 1, NP, FMT),                    \
      HFGRB2_ENTRY(3, 4, 2, 1, NP, FMT), HFGRB2_ENTRY(3, 2, 2, 1, NP, FMT)
EntryRb g_entriesRb2[] = {HFGRB2_SET(3, 0), HFGRB2_SET(3, 1), HFGRB2_SET(2, 1)};

template <size_t N>
EntryRb* find_in(EntryRb (&tab)[N], int C, int nwin, int wm, int kt, int np, int fmt,
                 bool persist) {
  for (auto& e : tab)
    if (e.kt == kt && e.C() == C && e.nwin() == nwin && e.wm == wm && e.np == np && e.fmt == fmt &&
        e.persist == persist)
      return &e;
  return nullptr;
}
EntryRb* find_rb(int C, int nwin, int wm, int kt, int np, int fmt, bool persist = false) {
  return find_in(g_entriesRb, C, nwin, wm, kt, np, fmt, persist);
}

}  // namespace

bool rb_supported(int C, int kt, int nwin, int wm) {
  return find_rb(C, nwin, wm, kt, 3, 0) != nullptr;
}

size_t rb_lds_bytes(int C, int nwin, int n_conv) { return rb_lds(C, nwin).total(n_conv); }

namespace {
// What both ResBlock launchers share once the instance is chosen: the window, halo and
// dilation-margin checks, the LDS size, the grid and the launch.
hipError_t launch_rb(EntryRb* e, const char* kernel, int C, int nwin, int kt, const RbParams& p,
                     int batch, hipStream_t stream, const char** name) {
  if (!e || p.n_conv > kRbMaxConv || batch < 1) return hipErrorInvalidValue;
  if (p.W <= 0 || p.halo < 0 || p.W + 2 * p.halo > nwin) return hipErrorInvalidValue;
  for (int i = 0; i < p.n_conv; ++i)
    if (p.dil[i] < 1 || (kt - 1) / 2 * p.dil[i] > rb_marg(C, nwin)) return hipErrorInvalidValue;
  const size_t lds = rb_lds_bytes(C, nwin, p.n_conv);
  const int n_tiles = (p.L + p.W - 1) / p.W;
  dim3 grid(n_tiles, batch);
  if (p.persist) {
    const int64_t n_win = (int64_t)n_tiles * batch;
    if (n_win >= (1ll << 31)) return hipErrorInvalidValue;
    grid = dim3((int)std::min<int64_t>(n_win, p.persist), 1);
  }
  auto fmt_name = [&](char* s, size_t n) {
    snprintf(s, n, "%s<%d, %d, %d, %d, %d, %d%s>", kernel, e->kt, e->waves_m, e->waves_n, e->wm,
             e->np, e->fmt, e->persist ? ", persist" : "");
  };
  return launch_instance(e->inst, fmt_name, grid, dim3(64 * e->waves_m * e->waves_n), lds, stream,
                         name, p);
}
}  // namespace

hipError_t launch_resblock_bf16x3(int C, int nwin, int wm, int kt, int fmt, int np,
                                  const RbParams& p_in, int batch, hipStream_t stream,
                                  const char** name) {
  RbParams p = p_in;
  p.batch = batch;
  // a persistent variant where one is built (one-block-per-CU shapes), else one window per block
  EntryRb* e = p.persist ? find_rb(C, nwin, wm, kt, np, fmt, true) : nullptr;
  if (!e) {
    p.persist = 0;
    e = find_rb(C, nwin, wm, kt, np, fmt);
  }
  // conv pairs from conv0 of the packed stream; the fused conv_post on C = 32, one window per block
  if (p.n_conv < 2 || (p.n_conv & 1)) return hipErrorInvalidValue;
  if (p.conv0 < 0 || p.conv0 + p.n_conv > p.n_conv_stream) return hipErrorInvalidValue;
  if (p.wav && (C != 32 || wm != 1 || p.L % 4 || p.W % 4 || p.halo < 4 || !p.post_w || !p.post_b ||
                p.amax_out || p.persist))
    return hipErrorInvalidValue;
  if (p.persist < 0) return hipErrorInvalidValue;
  return launch_rb(e, "resblock_bf16x3", C, nwin, kt, p, batch, stream, name);
}

bool rb2_supported(int C, int kt, int nwin, int wm) {
  return find_in(g_entriesRb2, C, nwin, wm, kt, 3, 0, false) != nullptr;
}

hipError_t launch_resblock2_bf16x3(int C, int nwin, int wm, int kt, int fmt, int np,
                                   const RbParams& p_in, int batch, hipStream_t stream,
                                   const char** name) {
  RbParams p = p_in;
  p.batch = batch;
  // the whole stream (any count from 1), one window per block, no fused conv_post
  if (p.n_conv < 1 || p.conv0 != 0 || p.n_conv_stream != p.n_conv) return hipErrorInvalidValue;
  if (p.wav || p.persist) return hipErrorInvalidValue;
  return launch_rb(find_in(g_entriesRb2, C, nwin, wm, kt, np, fmt, false), "resblock2_bf16x3", C,
                   nwin, kt, p, batch, stream, name);
}

}  // namespace hfg

#if HFG_RB_TIMING
HFG_TS_ENTRIES(rb, hfg::g_rb_ts, hfg::kRbTs)
#endif
