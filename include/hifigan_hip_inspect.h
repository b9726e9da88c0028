/*
 * hifigan_hip_inspect.h — host-only inspection entry points of
 * libhifigan_hip.so, used by the CPU test-suite to check weight packing
 * without a GPU.  Not part of the reference-facing boundary
 * (include/hifigan_hip.h); a handle created with device = -1 is host-only:
 * it validates the configuration, accepts hfg_set_weight with host data and
 * packs weights, but cannot run hfg_forward*.
 */
#ifndef HIFIGAN_HIP_INSPECT_H
#define HIFIGAN_HIP_INSPECT_H

#include <stddef.h>
#include <stdint.h>

#include "hifigan_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Copy the packed image of one layer (module prefix, e.g. "ups.0") into out:
 * w_len packed GEMM weights followed by b_len per-row biases.  info[10]
 * receives {kind (0 conv, 1 ups, 2 post), M, KT, tile, m_tiles, n_chunks,
 * w_len, b_len, CK, MT}.  With out == NULL only info is filled (no commit).
 * "<module>#small" selects the layer's second packing for the small-grid tile and
 * "<module>#frames" the output-frame upsampler's (info: M = rows per class C_out * u / 2,
 * KT = 2, tile = its configuration, n_chunks = channel groups, b_len = C_out); HFG_EINVAL
 * where the plan has no such packing. */
int hfg_debug_packed_layer(hfg_handle* h, const char* mod, float* out, size_t cap,
                           int64_t* info);

/* *ew <- the f16x3 packing exponent of layer `mod` (its split planes hold f16 halves of
 * w * 2^ew; 0 in the other modes).  Commits pending weights first and returns that
 * commit's error (HFG_EINVAL while a weight is missing). */
int hfg_debug_layer_exponent(hfg_handle* h, const char* mod, int* ew);

/* Packed image of the whole-ResBlock launch of stage `stage`, ResBlock `j`
 * (resblock_bf16x3.hip; split-precision handles, stages with 32, 64 or 128 channels):
 * w_len floats of A stream (hi/lo pairs of each conv's split format and exponent, as
 * hfg_debug_packed_layer of that conv reports) followed by b_len biases.
 * info[8] receives {fused (0/1), C, KT, n_conv, halo, W, w_len, b_len}.
 * Returns HFG_OK with info[0] = 0 when the stage runs layer by layer. */
int hfg_debug_packed_resblock(hfg_handle* h, int stage, int j, float* out, size_t cap,
                              int64_t* info);

/* The handle's plan as JSON in buf (NUL-terminated): per layer its kernel path, tile,
 * packings and packed-buffer offsets; per stage its thin-MRF launch; per ResBlock its
 * whole-block launch (window, halo, split, fused conv_post); the packed image's length in
 * floats and the sha256 of its bytes.  Everything the launch code reads from the plan, so
 * the host suite can pin it (tests/golden/plan_index.json).  Host-only handles included;
 * commits pending weights first and returns that commit's error.  HFG_EINVAL when buflen
 * is too small. */
int hfg_debug_plan(hfg_handle* h, char* buf, size_t buflen);

/* Window columns of the thin whole-MRF kernel of a C-channel stage (mfma == 0: mrf_thin,
 * mfma != 0: mrf_thin_mfma), which the plan does not list: a launch's centre is that window
 * less twice the stage's largest thin_halo.  0 when there is no such kernel. */
int hfg_debug_thin_window(int C, int mfma);

/* Dynamic-LDS bytes the launcher of a kernel family requests for a launch with the given
 * integer arguments (no handle, no device), so the host suite can pin every kernel's LDS
 * layout (tests/golden/lds_index.json).  family and args[n_args]:
 *   "conv_bf16x3"      {tile, taps, dilation, LDS-staged epilogue 0|1}
 *   "ups_bf16x3"       {configuration}
 *   "resblock_bf16x3"  {channels, window columns, convs of the launch}  (both ResBlock kernels)
 *   "mrf_thin", "mrf_thin_mfma"  {channels}
 *   "conv1d_mfma_f32"  {tile, taps, dilation}
 *   "conv_post"        {channels}
 *   "logmel_fft"       {n_fft, hop, n_mels, frames per wave}  (also release_mel_fft)
 *   "stft_power_mfma"  {n_fft, hop}  (-1 where hfg_mel_create refuses the DFT-GEMM pair)
 * -1 for an unknown family, a wrong argument count, or arguments the family has no kernel
 * for. */
int64_t hfg_debug_lds_bytes(const char* family, const int* args, int n_args);

/* The workspace layout of a forward as JSON in buf (NUL-terminated): what hfg_workspace_bytes
 * (hfg_mrf_workspace_bytes) totals and the launch schedule takes every pointer from.
 *   {"total": bytes, "parts": [{"b0", "B", "off", "bytes", "regions": [{"name", "off", "bytes"}]}]}
 * A generator handle (B, T frames): one part, or the two batch halves [b0, b0 + B) of a split
 * forward; per part the regions "X", "R", "Tb", "MRF", with concurrent ResBlocks "rb<j>.R",
 * "rb<j>.Tb", "rb<j>.out" per ResBlock, "table" (per-stage lengths) and "slots" (f16x3
 * scales, 0 bytes in the unscaled modes).  taps != 0: the layout hfg_forward_taps runs, the
 * whole batch as one part; its total never exceeds hfg_workspace_bytes, which covers both.
 * An MRF handle (B, L samples; taps ignored): one part of "R", "Tb" and "slots".  Offsets are
 * bytes from the workspace's start, 256-byte aligned.  Host-only handles included; no commit.
 * HFG_EINVAL when buflen is too small. */
int hfg_debug_workspace(const hfg_handle* h, int64_t B, int64_t T_or_L, int taps, char* buf,
                        size_t buflen);

/* A Generator forward (one stream) that also copies the stage outputs the
 * reference's forward passes through (models/hifigan.py:238-251) into
 * caller-owned device buffers: taps[0] <- conv_pre [B][C0][T], taps[1 + 2i] <-
 * ups[i] [B][C_i+1][L_i+1], taps[2 + 2i] <- mrfs[i] [B][C_i+1][L_i+1].
 * n_taps must be 1 + 2 * n_up; NULL entries are skipped. */
int hfg_forward_taps(hfg_handle* h, const float* mel, int64_t B, int64_t T, float* wav,
                     int64_t out_len, void* workspace, size_t workspace_bytes,
                     float* const* taps, int n_taps, void* stream);

/* Schedule overrides for A/B runs and the parity suites (process-wide; read by every
 * later hfg_create / hfg_mrf_create / hfg_mel_create / hfg_resample_create).  The library reads no environment
 * variable for its schedule (the HFG_* knobs of rounds 1-5 are only warned about), so a
 * production handle runs the default schedule whatever its process inherits.  Knobs:
 * FUSED_RB 0|1, FUSE_POST 0|1, RB_SPLIT 0|1, SMALL_TILE -1|0|1, RB_CONC -1|0|1,
 * UPS_FRAMES 1|2, SPLIT 1|2, RB_PERSIST 0..2, DEBUG_FLAGS (ablation builds), MEL_DFT 0|1,
 * AREG_TALL 0|1, RESAMPLE_TABLE 0|1 (hfg_resample_ragged's filter table: phase-major | tap-major).
 * set: HFG_EINVAL for an unknown knob or a value out of range.  clear: one knob, or all
 * with knob == NULL.  get: 1 and *value if the knob is overridden, 0 if not.
 * knob: the name of knob i of the library's table, NULL past its end. */
int hfg_debug_schedule_set(const char* knob, int value);
int hfg_debug_schedule_clear(const char* knob);
int hfg_debug_schedule_get(const char* knob, int* value);
const char* hfg_debug_schedule_knob(int i);

/* Sustained matrix-core rate of GPU `device` under a full-chip load (csrc/probe.hip):
 * 2 blocks x 4 waves per CU issue independent MFMAs back to back on random operands
 * that change every instruction, `iters` rounds of 32 MFMAs per wave (after a warm-up
 * launch of iters / 4).  kind 0: v_mfma_f32_32x32x16_bf16, kind 1:
 * v_mfma_f32_32x32x2_f32, 4 independent accumulator chains per wave; kinds 2 / 3: the
 * same with one chain (each MFMA accumulates onto the previous one's result; 8 MFMAs
 * per round instead of 32); kinds 4 / 5: v_mfma_f32_32x32x16_f16 (the f16x3 kernels'
 * instruction) on operands with random 10-bit mantissas, 4 chains / 1 chain.
 * *tflops <- dense TFLOP/s over the timed launch (HIP events),
 * *mhz <- shader clock over it (s_memtime against the 100 MHz real-time counter).
 * Measurement only (bench.py's roofline "peak_sustained"); synchronous. */
int hfg_probe_mfma_rate(int device, int kind, int iters, double* tflops, double* mhz);

#ifdef __cplusplus
}
#endif
#endif /* HIFIGAN_HIP_INSPECT_H */
