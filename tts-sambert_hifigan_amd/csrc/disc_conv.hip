// disc_conv.hip — the discriminators' middle layers (models/hifigan.py:286-616): a grouped,
// strided Conv along H of a [B][C][H][W] tensor as an implicit GEMM on the 16x16x32 matrix
// cores, bias and leaky_relu(0.1) fused.  W is the period of a PeriodDiscriminator's fold
// (its (k, 1) Conv2d) and 1 for a ScaleDiscriminator's Conv1d; the output is written as
// [B][C_out][H_out][W], the reference's feature-map layout.
//
// Arithmetic: f16x3 (bf16x3_common.h: mma3 with three products, lo*hi, hi*lo, hi*hi of f16
// halves of power-of-two scaled operands, fp32 accumulation).  The weights carry one exponent
// per layer (p.ew, from the layer's largest |weight|, applied by the packer); the activations
// one per staged chunk window: the block takes the window's largest magnitude (a first pass
// over the same loads), scales by 2^ex into [2^14, 2^15) and splits once, when it stages, not
// once per tap.  Each chunk multiplies into a fresh accumulator that is folded into the fp32
// total as fma(acc, 2^-(ex + ew), total).  The scale depends on the item's own values only,
// so an item's result does not depend on the batch around it.  (bf16x3, tried first, left
// 0.5 .. 1.7e-5 of a map's peak: inside the parity bar, but 2.5e-5 relative on the
// feature-matching distance of two near waves, whose bar is 1e-5.)
//
// Block: 256 threads, 4 waves.  It owns kDiscNt = 64 output positions (ho, w) of one band of
// TW = min(W, 16) columns — position n of the band is (ho, wl) = (n / TW, n % TW) — and
// 16 MSUB output channels of one group; wave v holds the 16 positions 16 v .. 16 v + 15 as
// the MFMA's columns and all MSUB 16-row tiles.  GEMM K runs over (chunk of CK = min(cig, 32)
// input channels, tap, channel octet): a k-step is four octets of 8 channels, octet
// o = 4 step + (lane >> 4) at tap o / O, channels 8 (o % O) .. + 7 of the chunk, O = CK / 8;
// octets past the last tap multiply zeros.
//
// LDS (one array, dynamic): 16 bytes for the four waves' window maxima, then the staged input
// window of one chunk as two planes (hi, lo) of [R rows][TW][CK + 8] halves,
// R = ceil(63 / TW) stride + k input rows from row (first ho) stride - pad; rows outside
// [0, H) and columns at or past W hold zeros (the zero padding: no padded copy).  The 8 spare
// halves per position keep 16-byte alignment and spread the positions over the banks.  A B fragment is one 16-byte read per plane.
//   bytes = 16 + 2 R TW (CK + 8) 2                             (disc_conv_lds_bytes)
// The A fragments are read from global (L2) in fragment order (disc_conv_nest, pack_layout.h).
//
// Instances: MSUB = 4 (64 rows: groups of 64 .. 1024 output channels), 2 (32) and 1 (16).
#include <hip/hip_runtime.h>

#include <cstdio>

#include "bf16x3_common.h"
#include "disc.h"
#include "launch.h"

namespace hfg {

namespace {

constexpr int kDiscFmt = kFmtF16;
constexpr int kDiscPadElems = 8;  // spare halves per staged position
constexpr int kDiscRedBytes = 16; // the waves' window maxima
__host__ __device__ constexpr int disc_pitch_bytes(int CK) { return (CK + kDiscPadElems) * 2; }

template <int MSUB>
__global__ void __launch_bounds__(256)
disc_conv_x3(DiscConvParams p, int TW, int bands, int R) {
  extern __shared__ __attribute__((aligned(16))) char lds_d[];
  const int cig = p.C_in / p.groups, cog = p.C_out / p.groups;
  const int CK = disc_conv_ck(cig), O = CK / 8;
  const int logO = O == 4 ? 2 : (O == 2 ? 1 : 0);
  const int chunks = cig / CK, steps = disc_conv_steps(cig, p.k);
  const int pitch = disc_pitch_bytes(CK);
  const int P = R * TW;                      // staged positions
  float* const red = reinterpret_cast<float*>(lds_d);
  char* const hi = lds_d + kDiscRedBytes;
  char* const lo = hi + (size_t)P * pitch;
  const int m_tiles = cog / (16 * MSUB);
  const int g = blockIdx.y / m_tiles, mt = blockIdx.y - g * m_tiles;
  const int tile = blockIdx.x / bands, band = blockIdx.x - tile * bands;
  const int b = blockIdx.z;
  const int w0 = band * TW;
  const int n0 = tile * kDiscNt;
  const int hfirst = n0 / TW;
  const int hin0 = hfirst * p.stride - p.pad;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // this lane's output position
  const int n = n0 + wave * 16 + (lane & 15);
  const int ho = n / TW, wl = n - ho * TW;
  const bool col_ok = ho < p.H_out && w0 + wl < p.W;
  // its window's first staged position; a position that stores nothing reads position 0
  const int pbase = col_ok ? (ho - hfirst) * p.stride * TW + wl : 0;
  const size_t HW = (size_t)p.H * p.W;
  const DiscConvPack pk = disc_conv_pack(MSUB);
  const bf16x8 zero8 = __builtin_bit_cast(bf16x8, floatx4_{0.f, 0.f, 0.f, 0.f});

  floatx4_ tot[MSUB];
#pragma unroll
  for (int m = 0; m < MSUB; ++m) tot[m] = floatx4_{0.f, 0.f, 0.f, 0.f};

  for (int c = 0; c < chunks; ++c) {
    if (c) lds_barrier();  // every wave has read the previous chunk's window
    // wave v takes the channel pairs v, v + 4, ..; a lane a position
    const float* xc = p.x + ((size_t)b * p.C_in + (size_t)g * cig + (size_t)c * CK) * HW;
    // first pass: the window's largest magnitude (NaNs drop out of fmaxf and travel on
    // through the split)
    float am = 0.f;
    for (int cp = wave; cp < CK / 2; cp += 4) {
      const float* x0 = xc + (size_t)(2 * cp) * HW;
      const float* x1 = x0 + HW;
      for (int pp = lane; pp < P; pp += 64) {
        const int r = TW == 1 ? pp : pp / TW;
        const int wc = pp - r * TW;
        const int hin = hin0 + r;
        if (hin >= 0 && hin < p.H && w0 + wc < p.W) {
          const size_t at = (size_t)hin * p.W + w0 + wc;
          am = fmaxf(am, fmaxf(fabsf(x0[at]), fabsf(x1[at])));
        }
      }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) am = fmaxf(am, __shfl_xor(am, m, 64));
    if (lane == 0) red[wave] = am;
    lds_barrier();
    const int ex = x3_exp(fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])));
    const float sx = exp2i(ex);
    floatx4_ acc[MSUB];
#pragma unroll
    for (int m = 0; m < MSUB; ++m) acc[m] = floatx4_{0.f, 0.f, 0.f, 0.f};
    // second pass: scale, split, stage
    for (int cp = wave; cp < CK / 2; cp += 4) {
      const float* x0 = xc + (size_t)(2 * cp) * HW;
      const float* x1 = x0 + HW;
      for (int pp = lane; pp < P; pp += 64) {
        const int r = TW == 1 ? pp : pp / TW;
        const int wc = pp - r * TW;
        const int hin = hin0 + r;
        float a0 = 0.f, a1 = 0.f;
        if (hin >= 0 && hin < p.H && w0 + wc < p.W) {
          const size_t at = (size_t)hin * p.W + w0 + wc;
          a0 = x0[at] * sx;
          a1 = x1[at] * sx;
        }
        bf16x2_ h2, l2;
        split_into<kDiscFmt>(a0, a1, h2, l2, 0);
        *reinterpret_cast<bf16x2_*>(hi + (size_t)pp * pitch + cp * 4) = h2;
        *reinterpret_cast<bf16x2_*>(lo + (size_t)pp * pitch + cp * 4) = l2;
      }
    }
    lds_barrier();
    prio_mfma();
    const __bf16* wch = p.w + (size_t)g * disc_conv_group_elems(cig, cog, p.k, MSUB) +
                        ((size_t)(mt * chunks + c) * steps) * pk.step + lane * pk.lane;
    for (int s = 0; s < steps; ++s) {
      const int o = 4 * s + (lane >> 4);
      const int tap = o >> logO, c8 = o & (O - 1);
      const int tc = tap < p.k ? tap : p.k - 1;
      const char* at = hi + (size_t)(pbase + tc * TW) * pitch + c8 * 16;
      bf16x8 bh = *reinterpret_cast<const bf16x8*>(at);
      bf16x8 bl = *reinterpret_cast<const bf16x8*>(at + (size_t)P * pitch);
      if (tap >= p.k) {  // an octet past the last tap: its weights are zeros, and so is this
        bh = zero8;
        bl = zero8;
      }
      const __bf16* ws = wch + (size_t)s * pk.step;
#pragma unroll
      for (int m = 0; m < MSUB; ++m) {
        const bf16x8 ah = *reinterpret_cast<const bf16x8*>(ws + m * pk.msub);
        const bf16x8 al = *reinterpret_cast<const bf16x8*>(ws + m * pk.msub + pk.plane);
        mma3<3, kDiscFmt>(ah, al, bh, bl, acc[m]);
      }
    }
    prio_other();
    const float sc = exp2i(-(ex + p.ew));
#pragma unroll
    for (int m = 0; m < MSUB; ++m)
#pragma unroll
      for (int j = 0; j < 4; ++j) tot[m][j] = __builtin_fmaf(acc[m][j], sc, tot[m][j]);
  }

  if (!col_ok) return;
  // C/D: column = lane & 15 (this lane's position), row = 4 (lane >> 4) + j
  const int row0 = g * cog + mt * 16 * MSUB + 4 * (lane >> 4);
  float* yb = p.y + (size_t)b * p.C_out * p.H_out * p.W + (size_t)ho * p.W + w0 + wl;
  const size_t HoW = (size_t)p.H_out * p.W;
#pragma unroll
  for (int m = 0; m < MSUB; ++m)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int co = row0 + 16 * m + j;
      float v = tot[m][j] + p.bias[co];
      if (p.act) v = lrelu3(v);
      yb[(size_t)co * HoW] = v;
    }
}

template <int MSUB>
hipError_t launch_msub(const DiscConvParams& p, int TW, int bands, int R, dim3 grid, size_t lds,
                       hipStream_t stream, const char** name) {
  static auto inst = instance_of(disc_conv_x3<MSUB>);
  auto fmt_name = [](char* s, size_t n) { snprintf(s, n, "disc_conv_x3<%d>", MSUB); };
  return launch_instance(inst, fmt_name, grid, dim3(256), lds, stream, name, p, TW, bands, R);
}

}  // namespace

int disc_conv_rows(int W, int k, int stride) {
  const int TW = disc_conv_tw(W);
  return (kDiscNt - 1 + TW - 1) / TW * stride + k;
}

size_t disc_conv_lds_bytes(int cig, int W, int k, int stride) {
  return kDiscRedBytes + 2 * (size_t)disc_conv_rows(W, k, stride) * disc_conv_tw(W) *
                             disc_pitch_bytes(disc_conv_ck(cig));
}

bool disc_conv_supported(const DiscConvParams& p) {
  if (p.groups < 1 || p.C_in < 1 || p.C_out < 1 || p.C_in % p.groups || p.C_out % p.groups)
    return false;
  const int cig = p.C_in / p.groups, cog = p.C_out / p.groups;
  if (!disc_conv_widths_ok(cig, cog, disc_conv_msub(cog))) return false;
  if (p.k < 1 || p.stride < 1 || p.pad < 0 || p.pad >= p.k || p.H < 1 || p.W < 1) return false;
  if (p.H + 2 * p.pad < p.k || p.H_out != (p.H + 2 * p.pad - p.k) / p.stride + 1) return false;
  if ((int64_t)p.H_out * p.W > INT32_MAX - 2 * kDiscNt) return false;
  return disc_conv_lds_bytes(cig, p.W, p.k, p.stride) <= kMaxLdsBytes;
}

hipError_t launch_disc_conv(const DiscConvParams& p, int batch, hipStream_t stream,
                            const char** name) {
  if (!disc_conv_supported(p) || batch < 1 || batch > 65535) return hipErrorInvalidValue;
  const int cig = p.C_in / p.groups, cog = p.C_out / p.groups;
  const int msub = disc_conv_msub(cog);
  const int TW = disc_conv_tw(p.W), bands = (p.W + TW - 1) / TW;
  const int R = disc_conv_rows(p.W, p.k, p.stride);
  const int64_t tiles = ((int64_t)p.H_out * TW + kDiscNt - 1) / kDiscNt;
  if (tiles * bands > INT32_MAX) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(tiles * bands), (unsigned)(p.groups * (cog / (16 * msub))),
                  (unsigned)batch);
  if (grid.y > 65535) return hipErrorInvalidValue;
  const size_t lds = disc_conv_lds_bytes(cig, p.W, p.k, p.stride);
  switch (msub) {
    case 4: return launch_msub<4>(p, TW, bands, R, grid, lds, stream, name);
    case 2: return launch_msub<2>(p, TW, bands, R, grid, lds, stream, name);
    default: return launch_msub<1>(p, TW, bands, R, grid, lds, stream, name);
  }
}

}  // namespace hfg
