// pack_layout.h — the global-memory layout of every kernel family's packed operands (the A
// streams and slabs, the fp32 weight orders) and of the biases that go with them, stated once.
// The plan takes every region's length from a layout's size, the packer (pack.cpp) writes
// through its nest, the kernel takes its strides from the same value, and the LDS copy of a
// slab (lds_layout.h) is sized from it: a level added here moves all of them.
// Included at the end of kernels.h (it needs the tile configurations declared there).
//
// As in lds_layout.h, what a kernel reads is a plain struct of ints filled by a constexpr
// function of the tile configuration, in the unit (bf16, bytes or floats, as named) of the
// pointer the kernel indexes; a term with a run-time input is a __host__ __device__ constexpr
// function of its own that returns one number.  The host side reads a layout as a PackNest:
// the levels outermost first, each with its extent, its stride in elements of the packed
// operand (bf16 or floats) and what one step along it adds to the GEMM coordinates
// (row, ci, tap, plane, conv) of the weight stored there.  nest.index(...) is the element
// offset of a coordinate; the *_floats functions are the size of a whole packing in floats of
// the packed buffer.  The static_asserts at the end check, for every tile configuration, that
// a nest is dense: the index of its last coordinate plus one is its size.
#pragma once

#include <initializer_list>

#include "kernels.h"

namespace hfg {

// what one step along a level adds: GEMM row, input channel, tap, plane (0 = hi, 1 = lo) and
// conv (which weight tensor of a multi-conv stream)
struct PackAt {
  int row, ci, tap, plane, conv;
};
struct PackDim {
  int n;           // extent
  size_t stride;   // elements
  PackAt step;
};
struct PackNest {
  static constexpr int kMax = 10;
  PackDim d[kMax] = {};
  int nd = 0;
  constexpr PackNest& dim(int n, size_t stride, PackAt step) {
    d[nd++] = PackDim{n, stride, step};
    return *this;
  }
  // element offset of the coordinate (c[0] outermost; one number per level)
  constexpr size_t index(std::initializer_list<int> c) const {
    size_t at = 0;
    int i = 0;
    for (int v : c) at += (size_t)v * d[i++].stride;
    return at;
  }
  constexpr size_t last() const {  // index of the last coordinate
    size_t at = 0;
    for (int i = 0; i < nd; ++i) at += (size_t)(d[i].n - 1) * d[i].stride;
    return at;
  }
  constexpr size_t count() const {  // elements: the product of the extents
    size_t m = 1;
    for (int i = 0; i < nd; ++i) m *= (size_t)d[i].n;
    return m;
  }
};
// the levels every MFMA A fragment of 32 rows ends in: [lane >> 5][lane & 31][8], the lane
// halves `half_ci` channels apart; `lane` = elements per lane
constexpr PackNest& pack_lanes32(PackNest& n, int lane, int half_ci) {
  return n.dim(2, 32 * (size_t)lane, {0, half_ci, 0, 0, 0}).dim(32, lane, {1, 0, 0, 0, 0});
}

// floats of the packed buffer that hold n bf16 / n bytes (every size below is even / a
// multiple of 4)
constexpr size_t pack_floats_of_bf16(size_t n) { return n / 2; }
constexpr size_t pack_floats_of_bytes(size_t n) { return n / 4; }

// ---- biases ----
// layer kernels: one per GEMM row, zero past M, padded to whole m-tiles; ResBlock and thin
// launches: [conv][C]; the output-frame upsampler: [C_out] (one conv); conv_post: [1]
constexpr size_t pack_bias_rows(int m_tiles, int MT) { return (size_t)m_tiles * MT; }
constexpr size_t pack_bias_convs(int n_conv, int C) { return (size_t)n_conv * C; }

// ---- conv1d_bf16x3 (conv_bf16x3.hip); bf16 ----
// [m_tile][g][tap group][tap][plane][wave_m][wm][lane][8]: row = m_tile MT + wave_m 32 WM +
// wm 32 + (lane & 31), ci = 16 g + 8 (lane >> 5) + e, tap = tap group TPC + tap (zero past kt)
struct ConvBf16x3Pack {
  int lane;      // a lane's 8 channels (16 B)
  int row_tile;  // 64 lanes: 32 rows x 16 channels
  int plane;     // WAVES_M x WM row tiles: the hi plane, then the lo plane
  int tap;       // hi + lo
  int slab;      // TPC taps: one chunk (16 channels x TPC taps), copied to LDS whole
};
constexpr ConvBf16x3Pack conv_bf16x3_pack(const Bf16x3Cfg& t) {
  ConvBf16x3Pack l{};
  l.lane = 8;
  l.row_tile = 64 * l.lane;
  l.plane = t.WAVES_M * t.WM * l.row_tile;
  l.tap = 2 * l.plane;
  l.slab = t.TPC * l.tap;
  return l;
}
// chunks of a layer: 16-channel groups x tap groups
constexpr int conv_bf16x3_groups(int C_in) { return (C_in + kBf16x3Ck - 1) / kBf16x3Ck; }
constexpr int conv_bf16x3_tap_groups(const Bf16x3Cfg& t, int kt) { return (kt + t.TPC - 1) / t.TPC; }
constexpr size_t conv_bf16x3_pack_floats(const Bf16x3Cfg& t, int m_tiles, int n_chunks) {
  return pack_floats_of_bf16((size_t)m_tiles * n_chunks * conv_bf16x3_pack(t).slab);
}
constexpr PackNest conv_bf16x3_nest(const Bf16x3Cfg& t, int m_tiles, int n_g, int n_tg) {
  const ConvBf16x3Pack l = conv_bf16x3_pack(t);
  PackNest n;
  n.dim(m_tiles, (size_t)n_g * n_tg * l.slab, {t.MT(), 0, 0, 0, 0});
  n.dim(n_g, (size_t)n_tg * l.slab, {0, kBf16x3Ck, 0, 0, 0});
  n.dim(n_tg, l.slab, {0, 0, t.TPC, 0, 0}).dim(t.TPC, l.tap, {0, 0, 1, 0, 0});
  n.dim(2, l.plane, {0, 0, 0, 1, 0});
  n.dim(t.WAVES_M, (size_t)t.WM * l.row_tile, {32 * t.WM, 0, 0, 0, 0});
  n.dim(t.WM, l.row_tile, {32, 0, 0, 0, 0});
  return pack_lanes32(n, l.lane, 8).dim(8, 1, {0, 1, 0, 0, 0});
}

// ---- ups_bf16x3 (ups_bf16x3.hip); bytes ----
// [m_tile][g][class][tap][plane][wave_m][wm][lane][8]: class row rr = m_tile MT + wave_m 32 WM
// + wm 32 + (lane & 31), ci = 16 g + 8 (lane >> 5) + e; the nest's tap is 2 class + tap (which
// kernel index that is: pack.cpp)
struct UpsPack {
  int lane;      // 16 B
  int row_tile;  // 64 lanes
  int plane;     // WAVES_M x WM row tiles
  int tap;       // hi + lo
  int cls;       // 2 taps
  int slab;      // 2 classes: one 16-channel group, copied to LDS whole
};
constexpr UpsPack ups_pack(const UpsCfg& t) {
  UpsPack l{};
  l.lane = 16;
  l.row_tile = 64 * l.lane;
  l.plane = t.WAVES_M * t.WM * l.row_tile;
  l.tap = 2 * l.plane;
  l.cls = 2 * l.tap;
  l.slab = 2 * l.cls;
  return l;
}
constexpr size_t ups_pack_floats(const UpsCfg& t, int m_tiles, int n_g) {
  return pack_floats_of_bytes((size_t)m_tiles * n_g * ups_pack(t).slab);
}
constexpr PackNest ups_nest(const UpsCfg& t, int m_tiles, int n_g) {
  const UpsPack l = ups_pack(t);
  PackNest n;
  n.dim(m_tiles, (size_t)n_g * l.slab / 2, {t.MT(), 0, 0, 0, 0});
  n.dim(n_g, l.slab / 2, {0, 16, 0, 0, 0});
  n.dim(2, l.cls / 2, {0, 0, 2, 0, 0}).dim(2, l.tap / 2, {0, 0, 1, 0, 0});
  n.dim(2, l.plane / 2, {0, 0, 0, 1, 0});
  n.dim(t.WAVES_M, (size_t)t.WM * l.row_tile / 2, {32 * t.WM, 0, 0, 0, 0});
  n.dim(t.WM, l.row_tile / 2, {32, 0, 0, 0, 0});
  return pack_lanes32(n, l.lane / 2, 8).dim(8, 1, {0, 1, 0, 0, 0});
}

// ---- resblock_bf16x3 / resblock2_bf16x3 (resblock_body.h); bytes ----
// [row tile][conv][g][tap][plane][lane][8]: row = 32 row tile + (lane & 31), ci = 16 g +
// 4 (lane >> 5) + (e & 3) + 8 (e >> 2) (the permuted channel order of the kernel's operand
// planes).  A k-step is one (conv, g, tap); a row tile holds the steps of every conv of the
// stream.
struct RbPack {
  int lane;   // 16 B
  int plane;  // 64 lanes
  int step;   // hi + lo: one k-step of one 32-row tile
};
constexpr RbPack rb_pack() { return RbPack{16, 64 * 16, 2 * 64 * 16}; }
constexpr int rb_pack_steps(int C, int kt) { return C / 16 * kt; }  // k-steps per conv
// bytes from one row tile to the next: `steps` k-steps, those of all the stream's convs
__host__ __device__ constexpr int rb_pack_row_tile(int steps) { return steps * rb_pack().step; }
constexpr size_t rb_pack_bytes(int C, int kt, int n_conv) {
  return (size_t)(C / 32) * rb_pack_row_tile(n_conv * rb_pack_steps(C, kt));
}
constexpr size_t rb_pack_floats(int C, int kt, int n_conv) {
  return pack_floats_of_bytes(rb_pack_bytes(C, kt, n_conv));
}
constexpr PackNest rb_nest(int C, int kt, int n_conv) {
  const RbPack l = rb_pack();
  const size_t step = l.step / 2, conv = rb_pack_steps(C, kt) * step;
  PackNest n;
  n.dim(C / 32, n_conv * conv, {32, 0, 0, 0, 0}).dim(n_conv, conv, {0, 0, 0, 0, 1});
  n.dim(C / 16, kt * step, {0, 16, 0, 0, 0}).dim(kt, step, {0, 0, 1, 0, 0});
  n.dim(2, l.plane / 2, {0, 0, 0, 1, 0});
  return pack_lanes32(n, l.lane / 2, 4).dim(2, 4, {0, 8, 0, 0, 0}).dim(4, 1, {0, 1, 0, 0, 0});
}

// ---- mrf_thin_mfma (mrf_thin_mfma.hip), C = 16; bytes ----
// per conv [step][plane][lane][8]: row = lane & 15, ci = 8 ((lane >> 4) & 1) + e,
// tap = 2 step + (lane >> 5) (zero past k).  The stream is the convs one after another; the
// plan keeps each conv's byte offset.
struct ThinMfmaPack {
  int lane;   // 16 B
  int plane;  // 64 lanes
  int step;   // hi + lo: one k-step (16 channels x 2 taps)
};
constexpr ThinMfmaPack thin_mfma_pack() { return ThinMfmaPack{16, 64 * 16, 2 * 64 * 16}; }
constexpr int thin_mfma_steps(int C, int k) { return (k + 32 / C - 1) / (32 / C); }  // per conv
constexpr size_t thin_mfma_conv_bytes(int C, int k) {
  return (size_t)thin_mfma_steps(C, k) * thin_mfma_pack().step;
}
constexpr PackNest thin_mfma_nest(int C, int k) {
  const ThinMfmaPack l = thin_mfma_pack();
  PackNest n;
  n.dim(thin_mfma_steps(C, k), l.step / 2, {0, 0, 32 / C, 0, 0}).dim(2, l.plane / 2, {0, 0, 0, 1, 0});
  n.dim(2, 32 * 8, {0, 0, 1, 0, 0}).dim(2, 16 * 8, {0, 8, 0, 0, 0}).dim(16, 8, {1, 0, 0, 0, 0});
  return n.dim(8, 1, {0, 1, 0, 0, 0});
}

// ---- conv1d_mfma_f32 (conv_kernels.hip); floats ----
// [m_tile][chunk][tap][kk][wave_m][lane][wm]: row = m_tile MT + wave_m 32 WM + wm 32 +
// (lane & 31), ci = chunk CK + 2 kk + (lane >> 5)
struct ConvF32Pack {
  int lane;    // WM row tiles
  int wave_m;  // 64 lanes
  int kk;      // WAVES_M waves: one MFMA k-step (2 channels)
  int tap;     // CK / 2 k-steps
};
constexpr ConvF32Pack conv_f32_pack(const TileCfg& t, int CK) {
  ConvF32Pack l{};
  l.lane = t.WM;
  l.wave_m = 64 * l.lane;
  l.kk = t.WAVES_M * l.wave_m;
  l.tap = CK / 2 * l.kk;
  return l;
}
// one weight slab (a chunk: MT rows x CK channels x kt taps), copied to LDS whole
__host__ __device__ constexpr int conv_f32_slab(int MT, int CK, int kt) { return MT * CK * kt; }
constexpr size_t conv_f32_pack_floats(const TileCfg& t, int CK, int kt, int m_tiles, int n_chunks) {
  return (size_t)m_tiles * n_chunks * conv_f32_slab(t.MT(), CK, kt);
}
constexpr PackNest conv_f32_nest(const TileCfg& t, int CK, int kt, int m_tiles, int n_chunks) {
  const ConvF32Pack l = conv_f32_pack(t, CK);
  const size_t slab = conv_f32_slab(t.MT(), CK, kt);
  PackNest n;
  n.dim(m_tiles, n_chunks * slab, {t.MT(), 0, 0, 0, 0}).dim(n_chunks, slab, {0, CK, 0, 0, 0});
  n.dim(kt, l.tap, {0, 0, 1, 0, 0}).dim(CK / 2, l.kk, {0, 2, 0, 0, 0});
  n.dim(t.WAVES_M, l.wave_m, {32 * t.WM, 0, 0, 0, 0});
  return pack_lanes32(n, l.lane, 1).dim(t.WM, 1, {32, 0, 0, 0, 0});
}

// ---- mrf_thin (mrf_thin.hip): per conv [tap][ci][co] (the C output channels of one
// (tap, ci) are one scalar load); floats ----
constexpr size_t thin_pack_floats(int C, int k) { return (size_t)k * C * C; }
constexpr PackNest thin_nest(int C, int k) {
  PackNest n;
  return n.dim(k, (size_t)C * C, {0, 0, 1, 0, 0}).dim(C, C, {0, 1, 0, 0, 0}).dim(C, 1, {1, 0, 0, 0, 0});
}

// ---- conv_post (conv_kernels.hip, and fused into the last ResBlock launch): [C][7]; floats ----
constexpr int kConvPostTaps = 7;
constexpr size_t conv_post_pack_floats(int C) { return (size_t)C * kConvPostTaps; }
constexpr PackNest conv_post_nest(int C) {
  PackNest n;
  return n.dim(C, kConvPostTaps, {0, 1, 0, 0, 0}).dim(kConvPostTaps, 1, {0, 0, 1, 0, 0});
}

// ---- disc_conv (disc_conv.hip): the discriminators' grouped, strided convs; 16-bit halves
// (f16x3: f16 hi and lo planes of the weights scaled by the layer's power of two) ----
// per group [m_tile][chunk][step][msub][plane][lane][8], the groups one after another: row
// (within the group) = 16 MSUB m_tile + 16 msub + (lane & 15); a k-step is four octets of
// 8 channels at one tap, octet o = 4 step + (lane >> 4): tap = o / O (zero past k),
// ci (within the group) = CK chunk + 8 (o % O) + e with CK = min(C_in / groups, 32) channels
// per chunk and O = CK / 8 octets per tap.
constexpr int kDiscCkMax = 32;
struct DiscConvPack {
  int lane;   // a lane's 8 channels (16 B)
  int plane;  // 64 lanes: 16 rows x 4 octets
  int msub;   // hi + lo: one 16-row tile of one k-step
  int step;   // MSUB row tiles
};
constexpr DiscConvPack disc_conv_pack(int MSUB) {
  DiscConvPack l{};
  l.lane = 8;
  l.plane = 64 * l.lane;
  l.msub = 2 * l.plane;
  l.step = MSUB * l.msub;
  return l;
}
__host__ __device__ constexpr int disc_conv_ck(int cig) { return cig < kDiscCkMax ? cig : kDiscCkMax; }
// group widths the layout holds: 8, 16 or a multiple of 32 input channels, whole 16-row tiles
constexpr bool disc_conv_widths_ok(int cig, int cog, int MSUB) {
  return (cig == 8 || cig == 16 || (cig > 0 && cig % 32 == 0)) && cog > 0 && cog % (16 * MSUB) == 0;
}
__host__ __device__ constexpr int disc_conv_steps(int cig, int k) {
  return (k * (disc_conv_ck(cig) / 8) + 3) / 4;
}
// 16-bit elements of one group's packing, and floats of a whole layer's
constexpr size_t disc_conv_group_elems(int cig, int cog, int k, int MSUB) {
  return (size_t)(cog / (16 * MSUB)) * (cig / disc_conv_ck(cig)) * disc_conv_steps(cig, k) *
         disc_conv_pack(MSUB).step;
}
constexpr size_t disc_conv_pack_floats(int cig, int cog, int k, int groups, int MSUB) {
  return pack_floats_of_bf16((size_t)groups * disc_conv_group_elems(cig, cog, k, MSUB));
}
constexpr PackNest disc_conv_nest(int cig, int cog, int k, int MSUB) {
  const DiscConvPack l = disc_conv_pack(MSUB);
  const int CK = disc_conv_ck(cig), O = CK / 8, steps = disc_conv_steps(cig, k);
  const int chunks = cig / CK;
  PackNest n;
  n.dim(cog / (16 * MSUB), (size_t)chunks * steps * l.step, {16 * MSUB, 0, 0, 0, 0});
  n.dim(chunks, (size_t)steps * l.step, {0, CK, 0, 0, 0});
  n.dim(steps, l.step, {0, 0, 4 / O, 0, 0}).dim(MSUB, l.msub, {16, 0, 0, 0, 0});
  n.dim(2, l.plane, {0, 0, 0, 1, 0});
  n.dim(4 / O, (size_t)O * 16 * l.lane, {0, 0, 1, 0, 0}).dim(O, 16 * l.lane, {0, 8, 0, 0, 0});
  return n.dim(16, l.lane, {1, 0, 0, 0, 0}).dim(8, 1, {0, 1, 0, 0, 0});
}

// ---- self-check: every nest is dense (last index + 1 = extents' product = the size) ----
constexpr bool pack_dense(const PackNest& n, size_t elems) {
  return n.last() + 1 == elems && n.count() == elems;
}
constexpr bool pack_layouts_dense() {
  bool ok = true;
  for (int i = 0; i < TILE_COUNT; ++i)
    for (int kt : {1, 2, 3, 5, 7, 11, 13})
      ok = ok && pack_dense(conv_f32_nest(kTiles[i], ck_for(dispatch_kt(kt), i), kt, 3, 5),
                            conv_f32_pack_floats(kTiles[i], ck_for(dispatch_kt(kt), i), kt, 3, 5));
  // (slot 0, the removed tile, included: its packing would be as regular as the others')
  for (int i = 0; i < kBf16x3Tiles_n; ++i)
    ok = ok && pack_dense(conv_bf16x3_nest(kBf16x3Tiles[i], 3, 5, 2),
                          2 * conv_bf16x3_pack_floats(kBf16x3Tiles[i], 3, 5 * 2));
  for (int i = 0; i < kUpsCfgs_n; ++i)
    ok = ok && pack_dense(ups_nest(kUpsCfgs[i], 3, 5), 2 * ups_pack_floats(kUpsCfgs[i], 3, 5));
  for (int C : {32, 64, 128})
    for (int kt : {3, 7, 11})
      ok = ok && pack_dense(rb_nest(C, kt, 6), 2 * rb_pack_floats(C, kt, 6));
  for (int k : {3, 5, 7})
    ok = ok && pack_dense(thin_mfma_nest(16, k), thin_mfma_conv_bytes(16, k) / 2) &&
         pack_dense(thin_nest(8, k), thin_pack_floats(8, k));
  for (int cig : {8, 16, 32, 64})
    for (int k : {5, 41})
      for (int MSUB : {1, 2, 4})
        ok = ok && pack_dense(disc_conv_nest(cig, 64, k, MSUB),
                              disc_conv_group_elems(cig, 64, k, MSUB));
  return ok && pack_dense(conv_post_nest(32), conv_post_pack_floats(32));
}
static_assert(pack_layouts_dense(), "a packed-operand nest is not dense");

}  // namespace hfg
