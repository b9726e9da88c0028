/*
 * hifigan_hip_relmel.h — the public HiFi-GAN release's mel front end on the device
 * (jik876/hifi-gan meldataset.mel_spectrogram), the analysis half that every released
 * generator_v1 / v2 / v3 checkpoint was trained against.  Included by hifigan_hip.h; the
 * entry points live in libhifigan_hip.so beside the hfg_mel_* ones, whose signatures,
 * hfg_mel_config layout and behaviour are unchanged.
 *
 *                        hfg_mel_* (reference, torchaudio)      hfg_relmel_* (release)
 *   padding              center=True: reflect n_fft/2 a side   center=False after an explicit
 *                                                              reflect pad of (n_fft-hop)/2
 *   frames for N samples N / hop + 1                           N / hop
 *   spectrum             power re^2 + im^2                     sqrt(re^2 + im^2 + 1e-9)
 *   filterbank           torchaudio melscale_fbanks (float32)  librosa.filters.mel (Slaney scale
 *                                                              and norm), float64, stored fp32
 *   compression          log10(mel + 1e-10)                    ln(max(mel, 1e-5))
 *
 * One kernel launch per batch (release_mel_fft: float64 FFT, magnitude, projection and log;
 * the output is the float32 rounding of the float64 result).  n_fft must be a power of two
 * >= 16 whose frame tile fits the LDS, and n_fft - hop_size even and >= 0; anything else is
 * refused at create with HFG_EINVAL (there is no DFT-GEMM fallback on this path).
 *
 * Ragged batches: `lengths` (device int32 [B], or NULL: every item has n_samples) gives each
 * item's valid samples.  Item b is framed as if it were alone with len_b samples (the
 * reflection at its end uses len_b), has len_b / hop frames when len_b > (n_fft-hop)/2 and
 * len_b >= hop (else 0), and its columns at or past that count hold (float) ln(clip_val), the
 * mel of digital silence.  The kernel clamps len_b into [0, n_samples] and every sample index
 * into [0, len_b - 1]: no length value makes it read outside the item's n_samples floats,
 * and samples at or past len_b are never read.  `frame_lengths` (device int32 [B], or NULL)
 * receives the frame counts, ready to be hfg_forward_opts.lengths of hfg_forward_ex.
 */
#ifndef HIFIGAN_HIP_RELMEL_H
#define HIFIGAN_HIP_RELMEL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hfg_relmel_handle hfg_relmel_handle;
typedef struct hfg_relmel_config {
    int32_t sampling_rate;   /* 22050  (the release's config.json keys)      */
    int32_t n_fft;           /* 1024                                         */
    int32_t hop_size;        /* 256                                          */
    int32_t win_size;        /* 1024                                         */
    int32_t num_mels;        /* 80                                           */
    float fmin, fmax;        /* 0, 8000; fmax <= 0: sampling_rate / 2 (the release's null) */
    float spec_eps;          /* 0: 1e-9                                      */
    float clip_val;          /* 0: 1e-5                                      */
} hfg_relmel_config;

/* device -1: a host-only handle (configuration checks, frame counts).  Errors are read with
 * hfg_mel_last_error().  The handle's default tables are the periodic Hann window of
 * win_size centred in n_fft and the librosa filterbank, both evaluated in double. */
int hfg_relmel_create(const hfg_relmel_config* cfg, int device, hfg_relmel_handle** out);
void hfg_relmel_destroy(hfg_relmel_handle* h);
/* Replace the window [n_fft] and the filterbank [n_fft/2+1][num_mels] (host pointers, fp32). */
int hfg_relmel_set_tables(hfg_relmel_handle* h, const float* window, const float* fb);
/* n_samples / hop; -1 if n_samples <= (n_fft - hop) / 2 or n_samples < hop */
int64_t hfg_relmel_frames(const hfg_relmel_handle* h, int64_t n_samples);
/* mel[B][num_mels][n_samples / hop] = release mel of wav[B][n_samples].  Asynchronous on the
 * caller's stream: no workspace, no allocation, no synchronisation (capturable into a
 * hipGraph).  A host-only handle, NULL wav or mel, B <= 0 or an n_samples with no frame:
 * HFG_EINVAL. */
int hfg_relmel_forward(hfg_relmel_handle* h, const float* wav, int64_t B, int64_t n_samples,
                       const int32_t* lengths, float* mel, int32_t* frame_lengths, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HIFIGAN_HIP_RELMEL_H */
