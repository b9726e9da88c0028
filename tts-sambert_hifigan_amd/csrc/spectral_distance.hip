// spectral_distance.hip — forward-only spectral distances on the device, ragged batches:
//
// mel_distance_fft<Front>: sum |d| and sum d^2 over d = mel(wav) - target, the mel formed as
//   logmel_fft / release_mel_fft form it (the same Front, frame tile, LDS staging, float64
//   Stockham FFT, real-FFT split, spectrum, band projection and finish: mel_fft_body.h) and
//   compared in LDS against a held target [B][n_mels][T]: no mel is written.  mel_fft_block is
//   left textually as it is (moving its pieces into helpers moves the registers of the two mel
//   kernels); the frame loop is restated in mel_distance_block below.
// stft_distance_fft<NK>: the same two sums over d = ln(|STFT a| + eps) - ln(|STFT b| + eps),
//   center=True reflect framing at the item's own length (models/losses.py:625-706,
//   compute_stft_loss, one resolution per launch).  The log magnitudes of a's frame stay in
//   NK registers per lane while b's frame goes through the FFT buffers.
// specdist_finish: item b's block partials -> sums[b][2].
//
// Determinism: no floating-point atomics.  A thread adds its entries in index order, a wave
// folds by a fixed xor butterfly, thread 0 adds the four waves in order and stores the block's
// pair in ws[b][block]; specdist_finish adds them lane-strided, then the same butterfly.  A
// block past the item's frames stores an exact 0.0 and x + 0.0 = x, so item b's sums are the
// bits of its solo run whatever the batch's width, and the workspace needs no initialisation.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#include "kernels.h"
#include "launch.h"
#include "mel_fft_body.h"
#include "mel_kernels.h"

namespace hfg {

namespace {

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// the block's pair: waves folded in order through `red` (LDS no wave uses any more; the caller
// has passed a __syncthreads since its last use)
__device__ __forceinline__ void block_fold(double s1, double s2, double* red,
                                           double* __restrict__ part) {
  s1 = wave_sum(s1);
  s2 = wave_sum(s2);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    red[2 * wave] = s1;
    red[2 * wave + 1] = s2;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    part[0] = ((red[0] + red[2]) + red[4]) + red[6];
    part[1] = ((red[1] + red[3]) + red[5]) + red[7];
  }
}

// The item's length clamped into [0, n_samp]: whatever lens holds, every index formed below
// stays inside the item's n_samp floats.
__device__ __forceinline__ int64_t item_len(const int32_t* __restrict__ lens, int b,
                                            int64_t n_samp) {
  return lens ? min(max((int64_t)lens[b], (int64_t)0), n_samp) : n_samp;
}

}  // namespace

// What a front's distance kernel is given beyond the shared arguments, and the Front of item
// b: framed as if alone with len samples, `frames` = the compared frames min(frames(len), T).
template <class Front>
struct DistFront;
template <>
struct DistFront<ReleaseMelFront> {
  struct Params {
    double spec_eps, clip;
  };
  static __device__ __forceinline__ ReleaseMelFront make(int n_fft, int hop, int64_t len, int T,
                                                         const Params& p) {
    const int pad = (n_fft - hop) / 2;
    const int frames = (len > pad && len >= hop) ? (int)min(len / hop, (int64_t)T) : 0;
    return {pad, len, frames, T, p.spec_eps, p.clip, 0.f};
  }
};
template <>
struct DistFront<LogMelFront> {
  struct Params {
    float eps, ln_base;
    int log_mode;
  };
  static __device__ __forceinline__ LogMelFront make(int n_fft, int hop, int64_t len, int T,
                                                     const Params& p) {
    const int frames = len > n_fft / 2 ? (int)min(len / hop + 1, (int64_t)T) : 0;
    return {n_fft / 2, len, frames, T, p.eps, p.ln_base, p.log_mode};
  }
};

// mel_fft_block (mel_fft_body.h) up to its exit pass, which here reads the target tile in the
// order the mel would have been stored and keeps two sums.  target: the item's [n_mels][T];
// part: the block's pair.
template <class Front>
__device__ __forceinline__ void mel_distance_block(
    const Front& F, const float* __restrict__ x, int n_fft, int hop, int fpw,
    const float* __restrict__ window, const cd* __restrict__ tw, const int* __restrict__ band,
    const float* __restrict__ bw, int n_mels, const float* __restrict__ target, int T,
    double* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) char lds_m[];
  const int N2 = n_fft / 2;
  const int fpb = mel_fft_fpb(fpw);
  const int span = mel_fft_span(fpb, hop, n_fft);
  cd* const bufs = reinterpret_cast<cd*>(lds_m);                        // [4 waves][2][N2]
  float* const sig = reinterpret_cast<float*>(lds_m + mel_fft_sig_off(N2));  // [span]
  float* const mel_s = sig + mel_fft_mel_idx(span);                     // [n_mels][fpb]
  const int f0 = blockIdx.x * fpb;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  if (f0 >= F.frames) {   // block-uniform: nothing of this item to compare (len may be 0)
    if (threadIdx.x == 0) {
      part[0] = 0.0;
      part[1] = 0.0;
    }
    return;
  }
  for (int i = threadIdx.x; i < span; i += 256) sig[i] = F.sample(x, (int64_t)f0 * hop - F.pad + i);
  __syncthreads();
  cd* A = bufs + (size_t)wave * 2 * N2;
  cd* Bf = A + N2;
  for (int fi = 0; fi < fpw; ++fi) {
    const int fl = wave * fpw + fi;
    if (f0 + fl >= F.frames) break;    // wave-uniform
    const float* fr = sig + fl * hop;
    for (int n = lane; n < N2; n += 64) {
      const float x0 = fr[2 * n] * window[2 * n], x1 = fr[2 * n + 1] * window[2 * n + 1];
      A[n] = {(double)x0, (double)x1};
    }
    wave_sync();
    cd* src = stockham_fft(A, Bf, N2, tw, lane);
    cd* dst = src == A ? Bf : A;
    double* P = reinterpret_cast<double*>(dst);
    for (int k = lane; k <= N2; k += 64) {
      const cd zk = src[k & (N2 - 1)];
      const cd zm = src[(N2 - k) & (N2 - 1)];
      const cd zc = {zm.x, -zm.y};
      const cd s_ = cadd(zk, zc), d_ = csub(zk, zc);
      const cd wd = cmul(tw[k], d_);
      const double re = 0.5 * (s_.x + wd.y), im = 0.5 * (s_.y - wd.x);
      P[k] = F.spectrum(re, im);
    }
    wave_sync();
    for (int m = lane; m < n_mels; m += 64) {
      const int lo = band[3 * m], hi = band[3 * m + 1], off = band[3 * m + 2];
      double acc = 0.0;
      for (int k = lo; k < hi; ++k) acc += (double)bw[off + k - lo] * P[k];
      mel_s[m * fpb + fl] = F.finish(acc);   // the float32 the front end would have stored
    }
    wave_sync();
  }
  __syncthreads();
  const int nf = min(fpb, F.frames - f0);   // compared columns of this block: f0 + fl < T
  double s1 = 0.0, s2 = 0.0;
  for (int i = threadIdx.x; i < n_mels * fpb; i += 256) {
    const int m = i / fpb, fl = i - m * fpb;
    if (fl < nf) {
      const double d = (double)mel_s[i] - (double)target[(int64_t)m * T + f0 + fl];
      s1 += fabs(d);
      s2 += d * d;
    }
  }
  block_fold(s1, s2, reinterpret_cast<double*>(lds_m), part);
}

template <class Front>
__global__ void __launch_bounds__(256)
mel_distance_fft(const float* __restrict__ wav, int64_t n_samp, const int32_t* __restrict__ lens,
                 int n_fft, int hop, int fpw, const float* __restrict__ window,
                 const cd* __restrict__ tw, const int* __restrict__ band,
                 const float* __restrict__ bw, int n_mels, typename DistFront<Front>::Params p,
                 const float* __restrict__ target, int T, double* __restrict__ ws,
                 int32_t* __restrict__ frames_out) {
  const int b = blockIdx.y;
  const Front F = DistFront<Front>::make(n_fft, hop, item_len(lens, b, n_samp), T, p);
  if (blockIdx.x == 0 && threadIdx.x == 0) frames_out[b] = F.frames;
  mel_distance_block(F, wav + (int64_t)b * n_samp, n_fft, hop, fpw, window, tw, band, bw, n_mels,
                     target + (int64_t)b * n_mels * T, T,
                     ws + 2 * ((int64_t)b * gridDim.x + blockIdx.x));
}

// one wave, one frame: (float) ln(|X[k]| + eps) of the windowed frame at fr, k = lane + 64 j
// (0 where k > N2, on both signals alike)
template <int NK>
__device__ __forceinline__ void frame_logmag(const float* fr, const float* __restrict__ window,
                                             cd* A, cd* Bf, int N2, const cd* __restrict__ tw,
                                             int lane, double eps, float (&out)[NK]) {
  for (int n = lane; n < N2; n += 64) {
    const float x0 = fr[2 * n] * window[2 * n], x1 = fr[2 * n + 1] * window[2 * n + 1];
    A[n] = {(double)x0, (double)x1};
  }
  wave_sync();
  const cd* src = stockham_fft(A, Bf, N2, tw, lane);
#pragma unroll
  for (int j = 0; j < NK; ++j) {
    const int k = lane + 64 * j;
    float v = 0.f;
    if (k <= N2) {
      const cd zk = src[k & (N2 - 1)];
      const cd zm = src[(N2 - k) & (N2 - 1)];
      const cd zc = {zm.x, -zm.y};
      const cd s_ = cadd(zk, zc), d_ = csub(zk, zc);
      const cd wd = cmul(tw[k], d_);
      const double re = 0.5 * (s_.x + wd.y), im = 0.5 * (s_.y - wd.x);
      v = (float)log(sqrt(re * re + im * im) + eps);
    }
    out[j] = v;
  }
  wave_sync();   // the buffers are free for the next frame
}

// NK: bins per lane, 64 (NK - 1) >= n_fft / 2 (the launcher picks the instance)
template <int NK>
__global__ void __launch_bounds__(256)
stft_distance_fft(const float* __restrict__ a, const float* __restrict__ b_, int64_t n_samp,
                  const int32_t* __restrict__ lens, int n_fft, int hop, int fpw,
                  const float* __restrict__ window, const cd* __restrict__ tw, double eps,
                  double* __restrict__ ws, int32_t* __restrict__ frames_out) {
  extern __shared__ __attribute__((aligned(16))) char lds_m[];
  const int N2 = n_fft / 2;
  const int fpb = mel_fft_fpb(fpw);
  const int span = mel_fft_span(fpb, hop, n_fft);
  cd* const bufs = reinterpret_cast<cd*>(lds_m);
  float* const sig_a = reinterpret_cast<float*>(lds_m + mel_fft_sig_off(N2));
  float* const sig_b = sig_a + stft_dist_sig_stride(span);
  const int b = blockIdx.y;
  const int f0 = blockIdx.x * fpb;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int64_t len = item_len(lens, b, n_samp);
  const int frames = len > N2 ? (int)(len / hop + 1) : 0;   // center=True; <= the grid's frames
  if (blockIdx.x == 0 && threadIdx.x == 0) frames_out[b] = frames;
  double* const part = ws + 2 * ((int64_t)b * gridDim.x + blockIdx.x);
  if (f0 >= frames) {
    if (threadIdx.x == 0) {
      part[0] = 0.0;
      part[1] = 0.0;
    }
    return;
  }
  // reflection at 0 and at the item's own length; never an index at or past len
  const LogMelFront F{N2, len, frames, frames, 0.f, 0.f, 0};
  const float* xa = a + (int64_t)b * n_samp;
  const float* xb = b_ + (int64_t)b * n_samp;
  for (int i = threadIdx.x; i < span; i += 256) {
    const int64_t g = (int64_t)f0 * hop - N2 + i;
    sig_a[i] = F.sample(xa, g);
    sig_b[i] = F.sample(xb, g);
  }
  __syncthreads();
  cd* A = bufs + (size_t)wave * 2 * N2;
  cd* Bf = A + N2;
  double s1 = 0.0, s2 = 0.0;
  for (int fi = 0; fi < fpw; ++fi) {
    const int fl = wave * fpw + fi;
    if (f0 + fl >= frames) break;    // wave-uniform
    float la[NK], lb[NK];
    frame_logmag<NK>(sig_a + fl * hop, window, A, Bf, N2, tw, lane, eps, la);
    frame_logmag<NK>(sig_b + fl * hop, window, A, Bf, N2, tw, lane, eps, lb);
#pragma unroll
    for (int j = 0; j < NK; ++j) {
      const double d = (double)la[j] - (double)lb[j];
      s1 += fabs(d);
      s2 += d * d;
    }
  }
  __syncthreads();
  block_fold(s1, s2, reinterpret_cast<double*>(lds_m), part);
}

// sums[b] = the item's nblk block pairs: lane-strided, then the butterfly.  Block = one wave.
__global__ void __launch_bounds__(64)
specdist_finish(const double* __restrict__ ws, int nblk, double* __restrict__ sums) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const double* p = ws + 2 * (int64_t)b * nblk;
  double s1 = 0.0, s2 = 0.0;
  for (int i = lane; i < nblk; i += 64) {
    s1 += p[2 * i];
    s2 += p[2 * i + 1];
  }
  s1 = wave_sum(s1);
  s2 = wave_sum(s2);
  if (lane == 0) {
    sums[2 * b] = s1;
    sums[2 * b + 1] = s2;
  }
}

// ---------------------------------------------------------------------------------------

int64_t specdist_blocks(int64_t frames, int fpw) {
  const int fpb = mel_fft_fpb(fpw);
  return frames < 1 ? 0 : (frames + fpb - 1) / fpb;
}

size_t specdist_workspace_bytes(int64_t B, int64_t frames, int fpw) {
  return 2 * sizeof(double) * (size_t)B * (size_t)specdist_blocks(frames, fpw);
}

size_t stft_distance_lds_bytes(int n_fft, int hop, int fpw) {
  return stft_dist_lds_total(n_fft, hop, fpw);
}

namespace {

bool dist_shape_ok(int64_t B, int n_fft, int hop, int fpw, int64_t frames) {
  return n_fft >= 16 && !(n_fft & (n_fft - 1)) && fpw >= 1 && hop >= 1 && B >= 1 && B <= 65535 &&
         frames >= 1 && frames <= INT32_MAX;
}

hipError_t finish(const double* ws, int64_t B, int nblk, double* sums, hipStream_t stream) {
  specdist_finish<<<dim3((unsigned)B), dim3(64), 0, stream>>>(ws, nblk, sums);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_release_mel_distance(const float* wav, int64_t B, int64_t n_samp,
                                       const int32_t* lens, int n_fft, int hop, int fpw,
                                       const float* window, const void* tw, const int* band,
                                       const float* bw, int n_mels, float spec_eps, float clip,
                                       const float* target, int64_t T, double* ws, double* sums,
                                       int32_t* frames, hipStream_t stream) {
  const int64_t n_cols = n_samp / hop;
  if (!dist_shape_ok(B, n_fft, hop, fpw, n_cols) || hop > n_fft || ((n_fft - hop) & 1) ||
      T < 1 || T > INT32_MAX)
    return hipErrorInvalidValue;
  static auto inst = instance_of(mel_distance_fft<ReleaseMelFront>);
  auto fmt_name = [](char* s, size_t n) { snprintf(s, n, "mel_distance_fft<ReleaseMelFront>"); };
  const int nblk = (int)specdist_blocks(n_cols, fpw);
  const DistFront<ReleaseMelFront>::Params p{(double)spec_eps, (double)clip};
  hipError_t e = launch_instance(inst, fmt_name, dim3((unsigned)nblk, (unsigned)B), dim3(256),
                                 logmel_fft_lds_bytes(n_fft, hop, fpw, n_mels), stream, nullptr,
                                 wav, n_samp, lens, n_fft, hop, fpw, window,
                                 reinterpret_cast<const cd*>(tw), band, bw, n_mels, p, target,
                                 (int)T, ws, frames);
  return e != hipSuccess ? e : finish(ws, B, nblk, sums, stream);
}

hipError_t launch_logmel_distance(const float* wav, int64_t B, int64_t n_samp,
                                  const int32_t* lens, int n_fft, int hop, int fpw,
                                  const float* window, const void* tw, const int* band,
                                  const float* bw, int n_mels, float eps, int log_mode,
                                  float ln_base, const float* target, int64_t T, double* ws,
                                  double* sums, int32_t* frames, hipStream_t stream) {
  const int64_t n_frames = n_samp > n_fft / 2 ? n_samp / hop + 1 : 0;
  if (!dist_shape_ok(B, n_fft, hop, fpw, n_frames) || T < 1 || T > INT32_MAX)
    return hipErrorInvalidValue;
  static auto inst = instance_of(mel_distance_fft<LogMelFront>);
  auto fmt_name = [](char* s, size_t n) { snprintf(s, n, "mel_distance_fft<LogMelFront>"); };
  const int nblk = (int)specdist_blocks(n_frames, fpw);
  const DistFront<LogMelFront>::Params p{eps, ln_base, log_mode};
  hipError_t e = launch_instance(inst, fmt_name, dim3((unsigned)nblk, (unsigned)B), dim3(256),
                                 logmel_fft_lds_bytes(n_fft, hop, fpw, n_mels), stream, nullptr,
                                 wav, n_samp, lens, n_fft, hop, fpw, window,
                                 reinterpret_cast<const cd*>(tw), band, bw, n_mels, p, target,
                                 (int)T, ws, frames);
  return e != hipSuccess ? e : finish(ws, B, nblk, sums, stream);
}

namespace {

template <int NK>
hipError_t launch_stft_nk(dim3 grid, size_t lds, hipStream_t stream, const float* a,
                          const float* b, int64_t n_samp, const int32_t* lens, int n_fft, int hop,
                          int fpw, const float* window, const cd* tw, double eps, double* ws,
                          int32_t* frames) {
  static auto inst = instance_of(stft_distance_fft<NK>);
  auto fmt_name = [](char* s, size_t n) { snprintf(s, n, "stft_distance_fft<%d>", NK); };
  return launch_instance(inst, fmt_name, grid, dim3(256), lds, stream, nullptr, a, b, n_samp,
                         lens, n_fft, hop, fpw, window, tw, eps, ws, frames);
}

}  // namespace

hipError_t launch_stft_distance(const float* a, const float* b, int64_t B, int64_t n_samp,
                                const int32_t* lens, int n_fft, int hop, int fpw,
                                const float* window, const void* tw, double eps, double* ws,
                                double* sums, int32_t* frames, hipStream_t stream) {
  const int64_t n_frames = n_samp > n_fft / 2 ? n_samp / hop + 1 : 0;
  if (!dist_shape_ok(B, n_fft, hop, fpw, n_frames) || n_fft > 2048 || !(eps > 0.0))
    return hipErrorInvalidValue;
  const int nblk = (int)specdist_blocks(n_frames, fpw);
  const dim3 grid((unsigned)nblk, (unsigned)B);
  const size_t lds = stft_distance_lds_bytes(n_fft, hop, fpw);
  const cd* t = reinterpret_cast<const cd*>(tw);
  hipError_t e;
  // bins 0..n_fft/2 over 64 lanes: n_fft / 128 + 1 registers per lane
  if (n_fft <= 128)
    e = launch_stft_nk<2>(grid, lds, stream, a, b, n_samp, lens, n_fft, hop, fpw, window, t, eps,
                          ws, frames);
  else if (n_fft <= 512)
    e = launch_stft_nk<5>(grid, lds, stream, a, b, n_samp, lens, n_fft, hop, fpw, window, t, eps,
                          ws, frames);
  else if (n_fft <= 1024)
    e = launch_stft_nk<9>(grid, lds, stream, a, b, n_samp, lens, n_fft, hop, fpw, window, t, eps,
                          ws, frames);
  else
    e = launch_stft_nk<17>(grid, lds, stream, a, b, n_samp, lens, n_fft, hop, fpw, window, t, eps,
                           ws, frames);
  return e != hipSuccess ? e : finish(ws, B, nblk, sums, stream);
}

}  // namespace hfg
