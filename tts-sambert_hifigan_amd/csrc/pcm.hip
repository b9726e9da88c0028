// pcm.hip — the PCM boundary of the public HiFi-GAN release on the device: what its data
// loader does before the mel front end (meldataset.py: 16-bit PCM / MAX_WAV_VALUE,
// librosa.util.normalize(audio) * 0.95) and what inference.py does after the Generator
// (audio * MAX_WAV_VALUE, int16).  Four HBM-streaming kernels, ragged like release_mel_fft:
// a per-item length (device int32 [B], or null = n_samples) clamped into [0, n_samples];
// samples at or past it are never read.
//
//   pcm_peak        peak[b] = max |x| over [0, len_b), one atomicMax per block on the bit
//                   pattern (non-negative floats order as unsigned integers, and a NaN's
//                   pattern lies above +inf's: a NaN sample makes its item's peak NaN)
//   pcm_to_float    int16 / float32 -> float32, optionally (v / peak_b) * gain in float64
//                   with one final rounding: the release's evaluation
//   pcm_offsets     exclusive prefix sum of the clamped lengths (one block)
//   pcm_from_float  sat16(round(x * 32768)), padded [B][n] or packed at offsets[b]
//
// Grid (ceil(n / kPcmChunk), B), 256 threads, no dynamic LDS.  A row whose first element
// (input and output both) lies on a 16-byte boundary moves in 16-byte loads and stores,
// kPcmGroup samples at a time, a group that straddles the length sample by sample; any other
// row (an odd n_samples of int16, a packed output row) runs the strided scalar loop.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>

#include "mel_kernels.h"

namespace hfg {

constexpr int kPcmThreads = 256;
constexpr int kPcmGroup = 8;       // samples per vector step: 16 B of int16, 2 x 16 B of float
constexpr int kPcmChunk = 4096;    // samples per block (a multiple of kPcmGroup * 2 bytes = 16)

struct alignas(16) S16x8 {
  int16_t v[8];
};
struct alignas(16) F32x4 {
  float v[4];
};

__device__ __forceinline__ int64_t item_len(const int32_t* lens, int b, int64_t n) {
  return lens ? min(max((int64_t)lens[b], (int64_t)0), n) : n;
}

__device__ __forceinline__ bool aligned16(const void* p) {
  return (reinterpret_cast<uintptr_t>(p) & 15) == 0;
}

__device__ __forceinline__ void load_group(const int16_t* p, int16_t (&s)[kPcmGroup]) {
  const S16x8 a = *reinterpret_cast<const S16x8*>(p);
#pragma unroll
  for (int k = 0; k < 8; ++k) s[k] = a.v[k];
}
__device__ __forceinline__ void load_group(const float* p, float (&s)[kPcmGroup]) {
  const F32x4 a = *reinterpret_cast<const F32x4*>(p);
  const F32x4 b = *reinterpret_cast<const F32x4*>(p + 4);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    s[k] = a.v[k];
    s[4 + k] = b.v[k];
  }
}
__device__ __forceinline__ void store_group(float* p, const float (&s)[kPcmGroup]) {
  F32x4 a, b;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    a.v[k] = s[k];
    b.v[k] = s[4 + k];
  }
  *reinterpret_cast<F32x4*>(p) = a;
  *reinterpret_cast<F32x4*>(p + 4) = b;
}
__device__ __forceinline__ void store_group(int16_t* p, const int16_t (&s)[kPcmGroup]) {
  S16x8 a;
#pragma unroll
  for (int k = 0; k < 8; ++k) a.v[k] = s[k];
  *reinterpret_cast<S16x8*>(p) = a;
}

// |x| as the bit pattern of a non-negative float32.  int16: the magnitude in int32
// (|-32768| = 32768) over 32768, exact.
__device__ __forceinline__ uint32_t mag_bits(int16_t s) {
  const int m = s < 0 ? -(int)s : (int)s;
  return __float_as_uint((float)m * (1.0f / 32768.0f));
}
__device__ __forceinline__ uint32_t mag_bits(float x) {
  return __float_as_uint(x) & 0x7fffffffu;
}

template <typename T>
__global__ void __launch_bounds__(kPcmThreads)
pcm_peak(const T* __restrict__ wav, int64_t n, const int32_t* __restrict__ lens,
         float* __restrict__ peak) {
  __shared__ uint32_t part[kPcmThreads / 64];
  const int b = blockIdx.y;
  const int64_t len = item_len(lens, b, n);
  const int64_t c0 = (int64_t)blockIdx.x * kPcmChunk;
  if (c0 >= len) return;  // block-uniform: the memset's 0 stands
  const int64_t c1 = min(c0 + kPcmChunk, len);
  const T* x = wav + (int64_t)b * n;
  uint32_t m = 0;
  int64_t i = c0;
  if (aligned16(x)) {  // c0 is a multiple of 16 bytes in either type: every group is aligned
    const int64_t groups = (c1 - c0) / kPcmGroup;
    for (int64_t g = threadIdx.x; g < groups; g += kPcmThreads) {
      T s[kPcmGroup];
      load_group(x + c0 + g * kPcmGroup, s);
#pragma unroll
      for (int k = 0; k < kPcmGroup; ++k) m = max(m, mag_bits(s[k]));
    }
    i += groups * kPcmGroup;
  }
  for (i += threadIdx.x; i < c1; i += kPcmThreads) m = max(m, mag_bits(x[i]));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o));
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    m = max(max(part[0], part[1]), max(part[2], part[3]));
    if (m) atomicMax(reinterpret_cast<unsigned int*>(peak) + b, m);
  }
}

// The release's value of one sample.  NORM: (float)(((double) v / d) * gain), v = s / 32768
// in float64 for int16 (exact) and (double) x for float32: a float64 division, a float64
// product and one rounding, as numpy evaluates audio / MAX_WAV_VALUE, normalize() and * 0.95.
template <bool NORM>
__device__ __forceinline__ float pcm_value(int16_t s, double d, double gain) {
  if (!NORM) return (float)s / 32768.0f;
  return (float)((((double)s / 32768.0) / d) * gain);
}
template <bool NORM>
__device__ __forceinline__ float pcm_value(float x, double d, double gain) {
  if (!NORM) return x;
  return (float)(((double)x / d) * gain);
}

// librosa.util.normalize leaves a vector whose peak is below the smallest normal number of
// its dtype undivided: float64 for the int16 path (of a float32 peak, only 0 is below it),
// float32 for float32 input.
__device__ __forceinline__ double peak_divisor(float p, int16_t) {
  return (double)p < DBL_MIN ? 1.0 : (double)p;
}
__device__ __forceinline__ double peak_divisor(float p, float) {
  return p < FLT_MIN ? 1.0 : (double)p;
}

template <typename T, bool NORM>
__global__ void __launch_bounds__(kPcmThreads)
pcm_to_float(const T* __restrict__ wav, int64_t n, const int32_t* __restrict__ lens,
             const float* __restrict__ peak, double gain, float* __restrict__ out) {
  const int b = blockIdx.y;
  const int64_t len = item_len(lens, b, n);
  const int64_t c0 = (int64_t)blockIdx.x * kPcmChunk;
  if (c0 >= n) return;
  const int64_t c1 = min(c0 + kPcmChunk, n);
  const T* x = wav + (int64_t)b * n;
  float* y = out + (int64_t)b * n;
  const double d = NORM ? peak_divisor(peak[b], T()) : 1.0;
  int64_t i = c0;
  if (aligned16(x) && aligned16(y)) {
    const int64_t groups = (c1 - c0) / kPcmGroup;
    for (int64_t g = threadIdx.x; g < groups; g += kPcmThreads) {
      const int64_t j = c0 + g * kPcmGroup;
      float r[kPcmGroup];
      if (j + kPcmGroup <= len) {
        T s[kPcmGroup];
        load_group(x + j, s);
#pragma unroll
        for (int k = 0; k < kPcmGroup; ++k) r[k] = pcm_value<NORM>(s[k], d, gain);
      } else {  // at or across the length: read below it only
#pragma unroll
        for (int k = 0; k < kPcmGroup; ++k)
          r[k] = j + k < len ? pcm_value<NORM>(x[j + k], d, gain) : 0.f;
      }
      store_group(y + j, r);
    }
    i += groups * kPcmGroup;
  }
  for (i += threadIdx.x; i < c1; i += kPcmThreads)
    y[i] = i < len ? pcm_value<NORM>(x[i], d, gain) : 0.f;
}

// offsets[0] = 0, offsets[b + 1] = len_0 + ... + len_b (clamped lengths): one block, each
// thread a contiguous run of items.
__global__ void __launch_bounds__(kPcmThreads)
pcm_offsets(const int32_t* __restrict__ lens, int B, int64_t n, int64_t* __restrict__ offsets) {
  __shared__ int64_t part[kPcmThreads];
  const int per = (B + kPcmThreads - 1) / kPcmThreads;
  const int lo = min((int)threadIdx.x * per, B), hi = min(lo + per, B);
  int64_t s = 0;
  for (int b = lo; b < hi; ++b) s += item_len(lens, b, n);
  part[threadIdx.x] = s;
  __syncthreads();
  int64_t acc = 0;
  for (int t = 0; t < (int)threadIdx.x; ++t) acc += part[t];
  if (threadIdx.x == 0) offsets[0] = 0;
  for (int b = lo; b < hi; ++b) {
    acc += item_len(lens, b, n);
    offsets[b + 1] = acc;
  }
}

// sat16(round(x * 32768)): the product is exact (a power of two), round is truncation
// toward zero (numpy's astype('int16') of in-range values) or to nearest even, NaN gives 0.
__device__ __forceinline__ int16_t pcm_quantize(float x, int nearest) {
  if (x != x) return 0;
  float q = x * 32768.0f;
  q = nearest ? rintf(q) : truncf(q);
  q = fminf(fmaxf(q, -32768.0f), 32767.0f);
  return (int16_t)(int)q;
}

__global__ void __launch_bounds__(kPcmThreads)
pcm_from_float(const float* __restrict__ wav, int64_t n, const int32_t* __restrict__ lens,
               int nearest, const int64_t* __restrict__ offsets, int16_t* __restrict__ out) {
  const int b = blockIdx.y;
  const int64_t len = item_len(lens, b, n);
  // padded: the whole row is written (0 past len); packed: len samples at offsets[b]
  const int64_t end = offsets ? len : n;
  const int64_t c0 = (int64_t)blockIdx.x * kPcmChunk;
  if (c0 >= end) return;
  const int64_t c1 = min(c0 + kPcmChunk, end);
  const float* x = wav + (int64_t)b * n;
  int16_t* y = offsets ? out + offsets[b] : out + (int64_t)b * n;
  int64_t i = c0;
  if (aligned16(x) && aligned16(y)) {
    const int64_t groups = (c1 - c0) / kPcmGroup;
    for (int64_t g = threadIdx.x; g < groups; g += kPcmThreads) {
      const int64_t j = c0 + g * kPcmGroup;
      int16_t r[kPcmGroup];
      if (j + kPcmGroup <= len) {
        float s[kPcmGroup];
        load_group(x + j, s);
#pragma unroll
        for (int k = 0; k < kPcmGroup; ++k) r[k] = pcm_quantize(s[k], nearest);
      } else {
#pragma unroll
        for (int k = 0; k < kPcmGroup; ++k)
          r[k] = j + k < len ? pcm_quantize(x[j + k], nearest) : (int16_t)0;
      }
      store_group(y + j, r);
    }
    i += groups * kPcmGroup;
  }
  for (i += threadIdx.x; i < c1; i += kPcmThreads)
    y[i] = i < len ? pcm_quantize(x[i], nearest) : (int16_t)0;
}

static bool pcm_grid(int64_t B, int64_t n, dim3* grid) {
  if (B < 1 || B > 65535 || n < 1) return false;
  const int64_t chunks = (n + kPcmChunk - 1) / kPcmChunk;
  if (chunks > INT32_MAX) return false;
  *grid = dim3((unsigned)chunks, (unsigned)B);
  return true;
}

hipError_t launch_pcm_peak(const void* wav, bool s16, int64_t B, int64_t n, const int32_t* lens,
                           float* peak, hipStream_t stream) {
  dim3 grid;
  if (!pcm_grid(B, n, &grid)) return hipErrorInvalidValue;
  if (s16)
    pcm_peak<int16_t><<<grid, kPcmThreads, 0, stream>>>(static_cast<const int16_t*>(wav), n,
                                                         lens, peak);
  else
    pcm_peak<float><<<grid, kPcmThreads, 0, stream>>>(static_cast<const float*>(wav), n, lens,
                                                       peak);
  return hipGetLastError();
}

hipError_t launch_pcm_to_float(const void* wav, bool s16, int64_t B, int64_t n,
                               const int32_t* lens, const float* peak, double gain, float* out,
                               hipStream_t stream) {
  dim3 grid;
  if (!pcm_grid(B, n, &grid)) return hipErrorInvalidValue;
  const int16_t* ws = static_cast<const int16_t*>(wav);
  const float* wf = static_cast<const float*>(wav);
  if (s16 && peak)
    pcm_to_float<int16_t, true><<<grid, kPcmThreads, 0, stream>>>(ws, n, lens, peak, gain, out);
  else if (s16)
    pcm_to_float<int16_t, false><<<grid, kPcmThreads, 0, stream>>>(ws, n, lens, peak, gain, out);
  else if (peak)
    pcm_to_float<float, true><<<grid, kPcmThreads, 0, stream>>>(wf, n, lens, peak, gain, out);
  else
    pcm_to_float<float, false><<<grid, kPcmThreads, 0, stream>>>(wf, n, lens, peak, gain, out);
  return hipGetLastError();
}

hipError_t launch_pcm_offsets(const int32_t* lens, int64_t B, int64_t n, int64_t* offsets,
                              hipStream_t stream) {
  if (B < 1 || B > 65535 || n < 1) return hipErrorInvalidValue;
  pcm_offsets<<<1, kPcmThreads, 0, stream>>>(lens, (int)B, n, offsets);
  return hipGetLastError();
}

hipError_t launch_pcm_from_float(const float* wav, int64_t B, int64_t n, const int32_t* lens,
                                 bool nearest, const int64_t* offsets, int16_t* out,
                                 hipStream_t stream) {
  dim3 grid;
  if (!pcm_grid(B, n, &grid)) return hipErrorInvalidValue;
  pcm_from_float<<<grid, kPcmThreads, 0, stream>>>(wav, n, lens, nearest ? 1 : 0, offsets, out);
  return hipGetLastError();
}

}  // namespace hfg
