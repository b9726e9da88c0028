/*
 * hifigan_hip_disc.h — the reference's discriminators (models/hifigan.py:286-616) as
 * forward-only networks on the device.  Included by hifigan_hip.h; the entry points live in
 * libhifigan_hip.so.  No gradients, no spectral norm.  Errors are read with
 * hfg_mel_last_error().
 *
 * One handle is one discriminator:
 *   HFG_DISC_PERIOD, arg = the period (>= 1): PeriodDiscriminator(period).  The wave [B][T] is
 *     folded to [H0 = ceil(T / period)][period] with the reference's right reflect pad
 *     (sample T + j reads T - 2 - j), then convs.0 .. convs.4 ((5, 1) kernels, stride 3, 3, 3,
 *     3, 1, leaky_relu 0.1) and conv_post ((3, 1), no activation): 6 maps [C][H][period].
 *   HFG_DISC_SCALE, arg = the poolings in front (0, 1 or 2 times AvgPool1d(4, 2, padding 2)):
 *     ScaleDiscriminator behind MultiScaleDiscriminator's pooling of its index.  convs.0 ..
 *     convs.6 and conv_post: 8 maps [C][L][1].
 * A map is [B][C][H][W] float32, exactly the reference's feature map; the last map is
 * conv_post's output, which is also the discriminator's score.
 *
 * Weights: hfg_disc_set_weight copies one tensor from HOST memory, already folded (g v / |v|),
 * under the reference's names: "convs.N.weight" ([C_out][C_in / groups][k], or the Conv2d's
 * [C_out][C_in][k][1]), "convs.N.bias", "conv_post.weight", "conv_post.bias".  An unknown key
 * or another shape is HFG_EINVAL.  hfg_disc_commit packs and uploads them (synchronous);
 * HFG_EAGAIN if a key was never set.
 *
 * hfg_disc_forward runs on the caller's stream, allocates nothing, does not synchronise and is
 * capturable; every launch is on that one stream.  Item b's maps do not depend on the other
 * items of the batch.
 *
 * hfg_disc_fm_sums: sums[b * num_maps + i] = sum |fake_i[b] - real_i[b]| over map i of item b,
 * float64, no floating-point atomics and a fixed order: item b's sums are bitwise those of a
 * call on item b alone, and every call repeats bitwise.  maps_real / maps_fake: num_maps
 * device pointers each, maps of a forward of B items of T samples.
 *
 * HFG_EINVAL before any launch: a NULL pointer, B outside [1, 65535], T < 1 (or over 2^28), a
 * period discriminator whose reflect pad does not fit (T % period != 0 and
 * period - T % period >= T: torch refuses it too), a workspace below *_workspace_bytes, a
 * forward before commit, a host-only handle (device -1: shapes and sizes only).
 */
#ifndef HIFIGAN_HIP_DISC_H
#define HIFIGAN_HIP_DISC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hfg_disc_handle hfg_disc_handle;

#define HFG_DISC_PERIOD 0
#define HFG_DISC_SCALE 1
#define HFG_DISC_MAX_MAPS 8

int hfg_disc_create(int kind, int arg, int device, hfg_disc_handle** out);
void hfg_disc_destroy(hfg_disc_handle* h);
int hfg_disc_set_weight(hfg_disc_handle* h, const char* key, const float* data,
                        const int64_t* shape, int ndim);
int hfg_disc_commit(hfg_disc_handle* h);
/* 6 (period) or 8 (scale); -1 for NULL */
int hfg_disc_num_maps(const hfg_disc_handle* h);
/* dims = (C, H, W) of map i for items of T samples */
int hfg_disc_map_shape(const hfg_disc_handle* h, int64_t T, int i, int64_t dims[3]);
/* the pooled waves of a scale discriminator; never 0 for valid arguments, 0 for invalid ones */
size_t hfg_disc_workspace_bytes(const hfg_disc_handle* h, int64_t B, int64_t T);
/* wav: [B][T] float32 on the device; maps: num_maps device pointers (host array) */
int hfg_disc_forward(hfg_disc_handle* h, const float* wav, int64_t B, int64_t T,
                     float* const* maps, void* workspace, size_t workspace_bytes, void* stream);

size_t hfg_disc_fm_workspace_bytes(const hfg_disc_handle* h, int64_t B);
int hfg_disc_fm_sums(hfg_disc_handle* h, int64_t B, int64_t T, const float* const* maps_real,
                     const float* const* maps_fake, double* sums, void* workspace,
                     size_t workspace_bytes, void* stream);

/* Inspection: layer i's (1 <= i < num_maps - 1) packed weights as the kernel reads them,
 * unpacked again to [C_out][C_in / groups][k] fp32: plane 0 the f16 high halves, plane 1 the
 * low halves, both scaled back by the layer's power of two.  n: the floats `out` holds.  After
 * hfg_disc_commit. */
int hfg_disc_debug_unpacked(const hfg_disc_handle* h, int layer, int plane, float* out, size_t n);

#ifdef __cplusplus
}
#endif
#endif /* HIFIGAN_HIP_DISC_H */
