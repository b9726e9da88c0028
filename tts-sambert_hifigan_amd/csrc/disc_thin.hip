// disc_thin.hip — the thin ends of the discriminators in fp32 on the vector unit (disc.h):
//   disc_entry   C_in = 1 entry convs (MPD: 1 -> 32, k 5, stride 3 through the period fold
//                with the reference's right reflect pad fused; MSD: 1 -> 128, k 15)
//   disc_post    conv_post, C -> 1, k 3, no activation
//   disc_pool    AvgPool1d(4, 2, padding 2), count_include_pad
//   disc_fm_*    the feature-matching sums, float64, no atomics
// Every sum runs in a fixed order that depends on the item alone.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "bf16x3_common.h"
#include "disc.h"

namespace hfg {

namespace {

// one thread per output (co, ho, w), positions fastest
__global__ void __launch_bounds__(256) disc_entry(DiscEntryParams p) {
  const int64_t N = (int64_t)p.H_out * p.W;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N * p.C_out) return;
  const int b = blockIdx.y;
  const int co = (int)(i / N);
  const int64_t n = i - co * N;
  const int ho = (int)(n / p.W), w = (int)(n - (int64_t)ho * p.W);
  const float* src = p.src + (int64_t)b * p.T;
  const float* wt = p.w + (int64_t)co * p.k;
  float acc = p.bias[co];
  for (int t = 0; t < p.k; ++t) {
    const int h = ho * p.stride + t - p.pad;
    if (h < 0 || h >= p.H) continue;
    int64_t at = (int64_t)h * p.W + w;
    if (at >= p.T) at = 2 * p.T - 2 - at;   // reflect: sample T + j reads T - 2 - j
    acc = __builtin_fmaf(wt[t], src[at], acc);
  }
  p.y[((int64_t)b * p.C_out + co) * N + n] = lrelu3(acc);
}

// 64 positions per block; wave v sums channels [v C / 4, (v + 1) C / 4) in order, thread
// (v = 0) adds the four parts in order
__global__ void __launch_bounds__(256)
disc_post(const float* __restrict__ x, int C, int H, int W, const float* __restrict__ w,
          const float* __restrict__ bias, float* __restrict__ y) {
  __shared__ float part[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t N = (int64_t)H * W;
  const int64_t n = (int64_t)blockIdx.x * 64 + lane;
  const int b = blockIdx.y;
  float acc = 0.f;
  if (n < N) {
    const int h = (int)(n / W);
    const bool up = h > 0, dn = h + 1 < H;
    const int c0 = (int)((int64_t)wave * C / 4), c1 = (int)((int64_t)(wave + 1) * C / 4);
    const float* xc = x + ((int64_t)b * C + c0) * N + n;
    for (int c = c0; c < c1; ++c, xc += N) {
      if (up) acc = __builtin_fmaf(w[3 * c], xc[-W], acc);
      acc = __builtin_fmaf(w[3 * c + 1], xc[0], acc);
      if (dn) acc = __builtin_fmaf(w[3 * c + 2], xc[W], acc);
    }
  }
  part[wave][lane] = acc;
  __syncthreads();
  if (wave == 0 && n < N)
    y[(int64_t)b * N + n] = bias[0] + (((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane]);
}

__global__ void __launch_bounds__(256)
disc_pool(const float* __restrict__ x, int64_t L, float* __restrict__ y) {
  const int64_t Lo = L / 2 + 1;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= Lo) return;
  const float* xb = x + (int64_t)blockIdx.y * L;
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int64_t at = 2 * i - 2 + j;
    if (at >= 0 && at < L) s += xb[at];
  }
  y[(int64_t)blockIdx.y * Lo + i] = s * 0.25f;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// block (blk, map, item): elements blk 256 + tid + j 256 kDiscFmBlocks in order, the wave
// butterfly, the four waves in order
__global__ void __launch_bounds__(256) disc_fm_partial(DiscFmArgs a, double* __restrict__ ws) {
  __shared__ double red[4];
  const int map = blockIdx.y, b = blockIdx.z;
  const int64_t n = a.n[map];
  const float* r = a.real[map] + (int64_t)b * n;
  const float* f = a.fake[map] + (int64_t)b * n;
  double s = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += 256 * kDiscFmBlocks)
    s += fabs((double)f[i] - (double)r[i]);
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0)
    ws[((int64_t)b * a.n_maps + map) * kDiscFmBlocks + blockIdx.x] =
        ((red[0] + red[1]) + red[2]) + red[3];
}

// one wave per (item, map): lane = block
__global__ void __launch_bounds__(64)
disc_fm_finish(const double* __restrict__ ws, double* __restrict__ sums) {
  static_assert(kDiscFmBlocks == 64, "one partial per lane");
  const int64_t pair = blockIdx.x;
  const double s = wave_sum(ws[pair * kDiscFmBlocks + threadIdx.x]);
  if (threadIdx.x == 0) sums[pair] = s;
}

}  // namespace

hipError_t launch_disc_entry(const DiscEntryParams& p, int batch, hipStream_t stream) {
  const int64_t total = (int64_t)p.H_out * p.W * p.C_out;
  const int64_t blocks = (total + 255) / 256;
  if (batch < 1 || batch > 65535 || total < 1 || blocks > INT32_MAX) return hipErrorInvalidValue;
  disc_entry<<<dim3((unsigned)blocks, (unsigned)batch), dim3(256), 0, stream>>>(p);
  return hipGetLastError();
}

hipError_t launch_disc_post(const float* x, int C_in, int H, int W, const float* w,
                            const float* bias, float* y, int batch, hipStream_t stream) {
  const int64_t blocks = ((int64_t)H * W + 63) / 64;
  if (batch < 1 || batch > 65535 || blocks < 1 || blocks > INT32_MAX) return hipErrorInvalidValue;
  disc_post<<<dim3((unsigned)blocks, (unsigned)batch), dim3(256), 0, stream>>>(x, C_in, H, W, w,
                                                                              bias, y);
  return hipGetLastError();
}

hipError_t launch_disc_pool(const float* x, int64_t L, float* y, int batch, hipStream_t stream) {
  const int64_t blocks = (L / 2 + 1 + 255) / 256;
  if (batch < 1 || batch > 65535 || L < 1 || blocks > INT32_MAX) return hipErrorInvalidValue;
  disc_pool<<<dim3((unsigned)blocks, (unsigned)batch), dim3(256), 0, stream>>>(x, L, y);
  return hipGetLastError();
}

hipError_t launch_disc_fm_sums(const DiscFmArgs& a, int batch, double* ws, double* sums,
                               hipStream_t stream) {
  if (batch < 1 || batch > 65535 || a.n_maps < 1 || a.n_maps > kDiscMaxMaps)
    return hipErrorInvalidValue;
  disc_fm_partial<<<dim3(kDiscFmBlocks, (unsigned)a.n_maps, (unsigned)batch), dim3(256), 0,
                    stream>>>(a, ws);
  if (hipError_t e = hipGetLastError()) return e;
  disc_fm_finish<<<dim3((unsigned)(batch * a.n_maps)), dim3(64), 0, stream>>>(ws, sums);
  return hipGetLastError();
}

}  // namespace hfg
