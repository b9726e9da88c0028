// fft_f64.h — float64 Stockham FFT device helpers of the one-launch mel kernels' block body
// (mel_fft_body.h: logmel_fft and release_mel_fft): complex doubles in LDS, in-register
// radix 2 / 4 / 8 butterflies, one wave per transform.  Device code only.
#pragma once

#include <hip/hip_runtime.h>

namespace hfg {

struct cd {
  double x, y;
};
__device__ __forceinline__ cd cmul(cd a, cd b) {
  return {a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x};
}
__device__ __forceinline__ cd cadd(cd a, cd b) { return {a.x + b.x, a.y + b.y}; }
__device__ __forceinline__ cd csub(cd a, cd b) { return {a.x - b.x, a.y - b.y}; }
__device__ __forceinline__ cd cmul_mi(cd a) { return {a.y, -a.x}; }  // (-i) a

// in-register DFT of R points: out[q] = sum_r v[r] e^{-2 pi i r q / R}
template <int R>
__device__ __forceinline__ void dft_r(cd (&v)[R]);
template <>
__device__ __forceinline__ void dft_r<2>(cd (&v)[2]) {
  const cd a = cadd(v[0], v[1]), b = csub(v[0], v[1]);
  v[0] = a;
  v[1] = b;
}
template <>
__device__ __forceinline__ void dft_r<4>(cd (&v)[4]) {
  const cd t0 = cadd(v[0], v[2]), t1 = csub(v[0], v[2]);
  const cd t2 = cadd(v[1], v[3]), t3 = cmul_mi(csub(v[1], v[3]));
  v[0] = cadd(t0, t2);
  v[2] = csub(t0, t2);
  v[1] = cadd(t1, t3);
  v[3] = csub(t1, t3);
}
template <>
__device__ __forceinline__ void dft_r<8>(cd (&v)[8]) {
  cd e[4] = {v[0], v[2], v[4], v[6]}, o[4] = {v[1], v[3], v[5], v[7]};
  dft_r<4>(e);
  dft_r<4>(o);
  constexpr double s = 0.70710678118654752440;
  o[1] = {s * (o[1].x + o[1].y), s * (o[1].y - o[1].x)};   // e^{-i pi/4}
  o[2] = cmul_mi(o[2]);                                      // e^{-i pi/2}
  o[3] = {s * (o[3].y - o[3].x), -s * (o[3].x + o[3].y)};  // e^{-3i pi/4}
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    v[q] = cadd(e[q], o[q]);
    v[q + 4] = csub(e[q], o[q]);
  }
}

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// one Stockham pass of radix R over an N2-point sequence: sub-transforms of Ns -> Ns * R
// points (twiddle e^{-2 pi i r k / (Ns R)} = tw[2 r k N2 / (Ns R) mod N], tw[t] =
// e^{-2 pi i t / N}, N = 2 N2)
template <int R>
__device__ __forceinline__ void stockham_pass(const cd* __restrict__ src, cd* __restrict__ dst,
                                              int N2, int Ns, const cd* __restrict__ tw,
                                              int lane) {
  const int nb = N2 / R;
  const int tstep = 2 * (N2 / (Ns * R));
  for (int j = lane; j < nb; j += 64) {
    const int k = j & (Ns - 1);
    cd v[R];
#pragma unroll
    for (int r = 0; r < R; ++r) v[r] = src[j + r * nb];
    if (Ns > 1) {
#pragma unroll
      for (int r = 1; r < R; ++r) v[r] = cmul(v[r], tw[(r * k * tstep) & (2 * N2 - 1)]);
    }
    dft_r<R>(v);
    const int base = (j - k) * R + k;
#pragma unroll
    for (int q = 0; q < R; ++q) dst[base + q * Ns] = v[q];
  }
}

// the N2-point complex FFT of src (mixed radix: 8, then 4 or 2), ping-ponging between the two
// LDS buffers; returns the buffer that holds the result (the other one is free)
__device__ __forceinline__ cd* stockham_fft(cd* src, cd* dst, int N2, const cd* __restrict__ tw,
                                            int lane) {
  int Ns = 1, rem = __builtin_ctz(N2);
  while (rem > 0) {
    if (rem >= 3) {
      stockham_pass<8>(src, dst, N2, Ns, tw, lane);
      Ns *= 8;
      rem -= 3;
    } else if (rem == 2) {
      stockham_pass<4>(src, dst, N2, Ns, tw, lane);
      Ns *= 4;
      rem -= 2;
    } else {
      stockham_pass<2>(src, dst, N2, Ns, tw, lane);
      Ns *= 2;
      rem -= 1;
    }
    wave_sync();
    cd* t = src;
    src = dst;
    dst = t;
  }
  return src;
}

}  // namespace hfg
