// resample.hip — polyphase sinc resampling (torchaudio.transforms.Resample): resample_sinc,
// rows of one length, and resample_ragged, the resampler in front of the release chain.
//
// resample_ragged: a padded batch of planar multi-channel items x[B][C][n], int16 or float32,
// each with its own length, to mono float32 y[B][n_out] at the handle's rate ratio, in one
// launch (include/hifigan_hip_resample.h).
//
// Per item b: len_b = lens[b] clamped into [0, n] (null lens: n), out_len_b =
// ceil(n_phases * len_b / stride).  For m < out_len_b every channel c gets resample_sinc's own
// sum: one sequential fp32 fmaf chain from 0.f over the klen taps of phase m % n_phases on
// channel c of the item, zero outside [0, len_b), an int16 sample entering as (float) s / 32768.  C = 1 stores that chain; C > 1 stores ((chain_0 + chain_1) + ...) / (float) C:
// the reference's order, resample every channel, then the mean over channels.  Outputs in
// [out_len_b, n_out) are 0 and out_lens[b] = out_len_b.  Samples at or past len_b are never
// read.
//
// Grid (ceil(n_out / 256), B), 256 threads.  A block stages the input span of its 256 outputs
// for all C channels in LDS (lds_layout.h), zeros where the span leaves [0, len_b); a block
// wholly at or past out_len_b loads nothing.  The filter table is read from global memory (it
// stays cache-resident) in one of two layouts holding the same numbers: phase-major
// [n_phases][klen], resample_sinc's, where the lanes of a wave (consecutive phases) load klen
// floats apart, or tap-major [klen][n_phases], where they load consecutive floats.  One table
// load feeds the chains of up to four channels.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"
#include "mel_kernels.h"

namespace hfg {

// Polyphase sinc resampling (torchaudio _apply_sinc_resample_kernel: conv1d of the padded
// signal with the [n_phases][klen] kernel at stride `stride`, phases interleaved).  A block
// owns 256 consecutive outputs; the input span they read (<= 256/n_phases*stride + klen
// samples) is staged in LDS once, zero outside [0, n), and every output is one dot product
// of klen taps: an HBM-bound stream (reads ~stride/n_phases inputs per output).
__global__ void __launch_bounds__(256)
resample_sinc(const float* __restrict__ x, int64_t n, int64_t n_out,
              const float* __restrict__ kern, int n_phases, int stride, int klen, int width,
              float* __restrict__ y) {
  extern __shared__ float xs[];
  const int b = blockIdx.y;
  const int64_t m0 = (int64_t)blockIdx.x * 256;
  const int64_t q0 = m0 / n_phases;                     // first output frame of the block
  const int64_t q1 = (min(m0 + 256, n_out) - 1) / n_phases;
  const int64_t s0 = q0 * stride - width;               // first input sample read
  const int span = (int)((q1 - q0) * stride + klen);
  const float* xb = x + (int64_t)b * n;
  for (int i = threadIdx.x; i < span; i += 256) {
    const int64_t g = s0 + i;
    xs[i] = (g >= 0 && g < n) ? xb[g] : 0.f;
  }
  __syncthreads();
  const int64_t m = m0 + threadIdx.x;
  if (m >= n_out) return;
  const int64_t q = m / n_phases;
  const int j = (int)(m - q * n_phases);
  const float* kr = kern + (int64_t)j * klen;
  const float* xr = xs + (q - q0) * stride;
  float acc = 0.f;
  for (int k = 0; k < klen; ++k) acc = fmaf(xr[k], kr[k], acc);
  y[(int64_t)b * n_out + m] = acc;
}

hipError_t launch_resample(const float* x, int64_t B, int64_t n, int64_t n_out,
                           const float* kern, int n_phases, int stride, int klen, int width,
                           float* y, hipStream_t stream) {
  const size_t lds = resample_lds_bytes(1, n_phases, stride, klen);
  if (lds > kResampleMaxLds) return hipErrorInvalidValue;
  dim3 grid((unsigned)((n_out + 255) / 256), (unsigned)B);
  resample_sinc<<<grid, dim3(256), lds, stream>>>(x, n, n_out, kern, n_phases, stride, klen,
                                                  width, y);
  return hipGetLastError();
}

__device__ __forceinline__ float rr_sample(int16_t s) { return (float)s / 32768.0f; }
__device__ __forceinline__ float rr_sample(float x) { return x; }

// G channels' chains side by side: xr = the first tap's sample of the first of them, cs floats
// between channels; kr = the phase's first tap, ks floats between taps
template <int G>
__device__ __forceinline__ void rr_chains(const float* xr, int cs, const float* __restrict__ kr,
                                          int64_t ks, int klen, float (&acc)[G]) {
#pragma unroll
  for (int g = 0; g < G; ++g) acc[g] = 0.f;
  for (int k = 0; k < klen; ++k) {
    const float w = kr[(int64_t)k * ks];
#pragma unroll
    for (int g = 0; g < G; ++g) acc[g] = fmaf(xr[g * cs + k], w, acc[g]);
  }
}

// sum = ((chain_0 + chain_1) + ...): the first chain starts the sum, every later one is added
template <int G>
__device__ __forceinline__ void rr_add(const float (&acc)[G], bool first, float* sum) {
#pragma unroll
  for (int g = 0; g < G; ++g) *sum = (first && g == 0) ? acc[0] : *sum + acc[g];
}

template <typename T, bool TAP_MAJOR>
__global__ void __launch_bounds__(256)
resample_ragged(const T* __restrict__ x, int C, int64_t n, const int32_t* __restrict__ lens,
                int64_t n_out, const float* __restrict__ kern, int n_phases, int stride, int klen,
                int width, float* __restrict__ y, int32_t* __restrict__ out_lens) {
  extern __shared__ __attribute__((aligned(16))) float xs[];  // [C][resample_span]
  const int b = blockIdx.y;
  const int64_t len = lens ? min(max((int64_t)lens[b], (int64_t)0), n) : n;
  const int64_t out_len = min((len * n_phases + stride - 1) / stride, n_out);
  if (blockIdx.x == 0 && threadIdx.x == 0 && out_lens) out_lens[b] = (int32_t)out_len;
  const int64_t m0 = (int64_t)blockIdx.x * 256;
  const int64_t m = m0 + threadIdx.x;
  float* yb = y + (int64_t)b * n_out;
  if (m0 >= out_len) {  // block-uniform: wholly past the item, nothing is read
    if (m < n_out) yb[m] = 0.f;
    return;
  }
  const int cs = resample_span(n_phases, stride, klen);
  const int64_t q0 = m0 / n_phases;                        // first output frame of the block
  const int64_t q1 = (min(m0 + 256, out_len) - 1) / n_phases;
  const int64_t s0 = q0 * stride - width;                  // first input sample read
  const int span = (int)((q1 - q0) * stride + klen);       // <= cs
  const T* xb = x + (int64_t)b * C * n;
  for (int c = 0; c < C; ++c) {
    const T* xc = xb + (int64_t)c * n;
    for (int i = threadIdx.x; i < span; i += 256) {
      const int64_t g = s0 + i;
      xs[c * cs + i] = (g >= 0 && g < len) ? rr_sample(xc[g]) : 0.f;
    }
  }
  __syncthreads();
  if (m >= n_out) return;
  if (m >= out_len) {
    yb[m] = 0.f;
    return;
  }
  const int64_t q = m / n_phases;
  const int j = (int)(m - q * n_phases);
  const float* kr = TAP_MAJOR ? kern + j : kern + (int64_t)j * klen;
  const int64_t ks = TAP_MAJOR ? n_phases : 1;
  const float* xr = xs + (q - q0) * stride;
  float sum = 0.f;
  int c = 0;
  for (; c + 4 <= C; c += 4) {
    float acc[4];
    rr_chains<4>(xr + c * cs, cs, kr, ks, klen, acc);
    rr_add<4>(acc, c == 0, &sum);
  }
  if (c + 2 <= C) {
    float acc[2];
    rr_chains<2>(xr + c * cs, cs, kr, ks, klen, acc);
    rr_add<2>(acc, c == 0, &sum);
    c += 2;
  }
  if (c < C) {
    float acc[1];
    rr_chains<1>(xr + c * cs, cs, kr, ks, klen, acc);
    rr_add<1>(acc, c == 0, &sum);
  }
  yb[m] = C == 1 ? sum : sum / (float)C;
}

hipError_t launch_resample_ragged(const void* x, bool s16, int64_t B, int64_t C, int64_t n,
                                  const int32_t* lens, int64_t n_out, const float* kern,
                                  bool tap_major, int n_phases, int stride, int klen, int width,
                                  float* y, int32_t* out_lens, hipStream_t stream) {
  if (B < 1 || B > 65535 || C < 1 || n < 1 || n_out < 1 || n > INT32_MAX || n_out > INT32_MAX)
    return hipErrorInvalidValue;
  const size_t lds = resample_lds_bytes(C, n_phases, stride, klen);
  if (lds > kResampleMaxLds) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((n_out + 255) / 256), (unsigned)B);
  const int16_t* xi = static_cast<const int16_t*>(x);
  const float* xf = static_cast<const float*>(x);
  const int c = (int)C;
  if (s16 && tap_major)
    resample_ragged<int16_t, true><<<grid, dim3(256), lds, stream>>>(
        xi, c, n, lens, n_out, kern, n_phases, stride, klen, width, y, out_lens);
  else if (s16)
    resample_ragged<int16_t, false><<<grid, dim3(256), lds, stream>>>(
        xi, c, n, lens, n_out, kern, n_phases, stride, klen, width, y, out_lens);
  else if (tap_major)
    resample_ragged<float, true><<<grid, dim3(256), lds, stream>>>(
        xf, c, n, lens, n_out, kern, n_phases, stride, klen, width, y, out_lens);
  else
    resample_ragged<float, false><<<grid, dim3(256), lds, stream>>>(
        xf, c, n, lens, n_out, kern, n_phases, stride, klen, width, y, out_lens);
  return hipGetLastError();
}

}  // namespace hfg
