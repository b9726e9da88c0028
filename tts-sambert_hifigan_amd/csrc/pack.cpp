// pack.cpp — the handle's weights in the operand orders the kernels read: weight-norm
// folded fp32 tensors -> h->packed_host at the offsets of the plan (plan.cpp).  Host only.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "disc.h"
#include "handle.h"

using hfg::kTiles;
using hfg::PackAt;
using hfg::PackDim;
using hfg::PackNest;

namespace hfg_host {

namespace {

// float -> bf16, round to nearest even (NaN stays NaN)
inline uint16_t f2bf(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
inline float bf2f(uint16_t b) {
  uint32_t u = (uint32_t)b << 16;
  float f;
  memcpy(&f, &u, 4);
  return f;
}
// float -> f16 bits, round to nearest even (subnormals kept)
inline uint16_t f2h(float f) {
  const _Float16 h = (_Float16)f;
  uint16_t u;
  memcpy(&u, &h, 2);
  return u;
}
inline float h2f(uint16_t u) {
  _Float16 h;
  memcpy(&h, &u, 2);
  return (float)h;
}
// f16x3 exponent of a tensor with max |value| m: m 2^e in [2^14, 2^15), clamped like the
// device's x3_exp (bf16x3_common.h)
int x3_exp_host(float m) {
  if (!(m > 0.f) || !std::isfinite(m)) return 0;
  int x = 0;
  std::frexp(m, &x);
  return std::min(std::max(15 - x, -hfg::kX3ExpMax), hfg::kX3ExpMax);
}
// how one layer's weights are split into the kernels' (hi, lo) planes
struct WSplit {
  int fmt;      // hfg::kFmtBf16 / kFmtF16
  float scale;  // 2^ew (f16)
};
inline WSplit wsplit(const hfg_handle* h, const Layer& L) {
  return WSplit{h->fmt, std::ldexp(1.0f, L.ew)};
}
// plane 0: the high half of v, plane 1: the low half
inline uint16_t split_w(float v, const WSplit& ws, int plane) {
  if (ws.fmt == hfg::kFmtBf16) {
    const uint16_t hi = f2bf(v);
    return plane == 0 ? hi : f2bf(v - bf2f(hi));
  }
  const float a = v * ws.scale;  // exact (power of two)
  const uint16_t hi = f2h(a);
  return plane == 0 ? hi : f2h(a - h2f(hi));
}

const float* weight_of(hfg_handle* h, const Layer& L) {
  return h->params[L.mod + ".weight"].data.data();
}
const float* bias_of(hfg_handle* h, const Layer& L) {
  return h->params[L.mod + ".bias"].data.data();
}
uint16_t* halves_at(hfg_handle* h, size_t off) {
  return reinterpret_cast<uint16_t*>(h->packed_host.data() + off);
}

// Every element of a nest (pack_layout.h): f(its element offset, the GEMM coordinate of the
// weight stored there).  The innermost level is a plain loop, the outer ones an odometer.
template <typename F>
void for_each_packed(const PackNest& n, F f) {
  auto add = [](PackAt& a, const PackAt& s, int m) {
    a.row += m * s.row, a.ci += m * s.ci, a.tap += m * s.tap, a.plane += m * s.plane;
    a.conv += m * s.conv;
  };
  const PackDim& in = n.d[n.nd - 1];
  int c[PackNest::kMax] = {};
  size_t off = 0;
  PackAt at{};
  for (int d = 0; d >= 0;) {
    size_t o = off;
    PackAt a = at;
    for (int i = 0; i < in.n; ++i, o += in.stride, add(a, in.step, 1)) f(o, a);
    // the next coordinate of the outer levels: carry out of every level that wraps
    for (d = n.nd - 2; d >= 0; --d) {
      const PackDim& D = n.d[d];
      off += D.stride, add(at, D.step, 1);
      if (++c[d] < D.n) break;
      off -= D.n * D.stride, add(at, D.step, -D.n), c[d] = 0;
    }
  }
}
// fp32 operands: dst[offset] = wt(coordinate)
template <typename F>
void fill_f32(const PackNest& n, float* dst, F wt) {
  for_each_packed(n, [&](size_t i, const PackAt& a) { dst[i] = wt(a); });
}
// split operands: plane 0 / 1 of wt(coordinate), split as its conv's ws[conv] says
template <typename F>
void fill_split(const PackNest& n, uint16_t* dst, const WSplit* ws, F wt) {
  for_each_packed(n, [&](size_t i, const PackAt& a) { dst[i] = split_w(wt(a), ws[a.conv], a.plane); });
}
// biases [conv][C] of `convs` at region b
void pack_conv_biases(hfg_handle* h, const std::vector<int>& convs, int C, const PackRegion& b) {
  for (size_t e = 0; e < convs.size(); ++e)
    std::copy_n(bias_of(h, h->layers[convs[e]]), C,
                h->packed_host.data() + b.off + hfg::pack_bias_convs((int)e, C));
}

// mrf_thin weights (thin_nest) and, split precisions, the mrf_thin_mfma A stream
// (thin_mfma_nest; taps past k carry zeros)
void pack_thin(hfg_handle* h, const Stage& st) {
  const int C = st.C;
  for (size_t e = 0; e < st.thin_convs.size(); ++e) {
    const Layer& L = h->layers[st.thin_convs[e]];
    const float* w = weight_of(h, L);  // [C_out][C_in][k]
    auto wt = [&](const PackAt& a) { return a.tap < L.k ? w[((size_t)a.row * C + a.ci) * L.k + a.tap] : 0.f; };
    fill_f32(hfg::thin_nest(C, L.k), h->packed_host.data() + st.thin_w[e].off, wt);
    if (!st.thin_mfma) continue;
    const WSplit ws = wsplit(h, L);
    fill_split(hfg::thin_mfma_nest(C, L.k), halves_at(h, st.thin_m.off) + st.thin_m_conv[e] / 2, &ws, wt);
  }
  pack_conv_biases(h, st.thin_convs, C, st.thin_b);
}

// The A stream of a whole-ResBlock launch (rb_nest): every conv's nn.Conv1d weight
// [C_out][C_in][k], each split with its own exponent.  Biases [conv][C].
void pack_resblock(hfg_handle* h, const RbFused& rb) {
  const int C = h->layers[rb.convs[0]].C_out, KT = rb.kt;
  std::vector<const float*> w;
  std::vector<WSplit> ws;
  for (int cv : rb.convs) {
    w.push_back(weight_of(h, h->layers[cv]));
    ws.push_back(wsplit(h, h->layers[cv]));
  }
  fill_split(hfg::rb_nest(C, KT, (int)rb.convs.size()), halves_at(h, rb.w.off), ws.data(),
             [&](const PackAt& a) { return w[a.conv][((size_t)a.row * C + a.ci) * KT + a.tap]; });
  pack_conv_biases(h, rb.convs, C, rb.b);
}

// A slabs of the output-frame upsampler (ups_nest): class row rr -> co = rr / h, s' = rr % h
// (h = u/2); kernel index (nn.ConvTranspose1d weight [C_in][C_out][k]): class L (c = 0) tap 0
// (x[m-1]) s'+h+u, tap 1 (x[m]) s'+h; class R (c = 1) tap 0 (x[m]) s'+u, tap 1 (x[m+1]) s'.
// Bias [C_out].
void pack_ups_frames(hfg_handle* h, const Layer& L) {
  const float* w = weight_of(h, L);
  const WSplit ws = wsplit(h, L);
  const int u = L.s, hh = u / 2, k = L.k, cout = L.C_out;
  fill_split(hfg::ups_nest(hfg::kUpsCfgs[L.ups_cfg], L.m_tiles_f, L.C_in / 16), halves_at(h, L.wf.off),
             &ws, [&](const PackAt& a) {
               const int co = a.row / hh, sp = a.row % hh, c = a.tap >> 1, tp = a.tap & 1;
               const int j = c == 0 ? (tp == 0 ? sp + hh + u : sp + hh) : (tp == 0 ? sp + u : sp);
               return w[((size_t)a.ci * cout + co) * k + j];
             });
  std::copy_n(bias_of(h, L), cout, h->packed_host.data() + L.bf.off);
}

void pack_layer(hfg_handle* h, const Layer& L) {
  const float* w = weight_of(h, L);
  const float* bias = bias_of(h, L);
  float* packed = h->packed_host.data();
  // The GEMM weight at (row, ci, tap), zero outside [0, M) x [0, C_in) x [0, KT).  Conv1d and
  // conv_post: nn.Conv1d weight [C_out][C_in][k].  Polyphase ConvTranspose1d: row m = co*s + r;
  // tap jj reads x[u - (Q-1) + jj], i.e. original kernel index r + s*(Q-1-jj) of the
  // nn.ConvTranspose1d weight [C_in][C_out][k].
  const int cin = L.C_in, cout = L.C_out, k = L.k, s = L.kind == L_UPS ? L.s : 1, Q = L.KT;
  auto wt = [&](const PackAt& a) {
    if (a.row >= L.M || a.ci >= cin || a.tap >= Q) return 0.f;
    if (L.kind != L_UPS) return w[((size_t)a.row * cin + a.ci) * k + a.tap];
    const int co = a.row / s, r = a.row % s;
    const int kidx = r + s * (Q - 1 - a.tap);
    return kidx < k ? w[((size_t)a.ci * cout + co) * k + kidx] : 0.f;
  };
  if (L.kind == L_POST) {
    fill_f32(hfg::conv_post_nest(cin), packed + L.pk[0].w.off, wt);
    packed[L.pk[0].b.off] = bias[0];
    return;
  }
  // the layer's tile, then (split-precision layers with one) the small-grid tile
  for (const Packing& pk : L.pk) {
    if (pk.tile < 0) continue;
    if (L.prec == 1) {
      const hfg::Bf16x3Cfg& t = hfg::kBf16x3Tiles[pk.tile];
      const WSplit ws = wsplit(h, L);
      fill_split(hfg::conv_bf16x3_nest(t, pk.m_tiles, hfg::conv_bf16x3_groups(cin),
                                       hfg::conv_bf16x3_tap_groups(t, Q)),
                 halves_at(h, pk.w.off), &ws, wt);
    } else {
      fill_f32(hfg::conv_f32_nest(kTiles[pk.tile], L.CK, Q, pk.m_tiles, pk.n_chunks),
               packed + pk.w.off, wt);
    }
    for (size_t m = 0; m < pk.b.len; ++m) packed[pk.b.off + m] = m < (size_t)L.M ? bias[m / s] : 0.f;
  }
  if (L.ups_cfg >= 0) pack_ups_frames(h, L);
}

}  // namespace

int pack_weights(hfg_handle* h) {
  for (auto& key : h->param_order)
    if (!h->params[key].set) return fail(HFG_EAGAIN, "weight '%s' was never set", key.c_str());
  if (h->cfg.dtype == HFG_DTYPE_BF16W) {
    // bf16 weight storage: every conv weight rounded to bf16 (round-to-nearest-even) in
    // place, so every kernel (split planes: lo = 0; fp32 / VALU paths) sees the same
    // bf16-valued weights; biases stay fp32.  Idempotent across commits.
    for (auto& kv : h->params) {
      const std::string& k = kv.first;
      if (k.size() < 7 || k.compare(k.size() - 7, 7, ".weight") != 0) continue;
      for (float& v : kv.second.data) v = bf2f(f2bf(v));
    }
  }
  std::fill(h->packed_host.begin(), h->packed_host.end(), 0.f);
  // f16x3 weight scales: one power of two per layer, from its largest |weight|
  for (auto& L : h->layers) {
    L.ew = 0;
    if (h->fmt != hfg::kFmtF16 || L.kind == L_POST) continue;
    float m = 0.f;
    for (float v : h->params[L.mod + ".weight"].data) m = std::max(m, std::fabs(v));
    L.ew = x3_exp_host(m);
  }
  for (auto& L : h->layers) pack_layer(h, L);
  for (auto& st : h->stages) {
    for (auto& rb : st.rbs)
      if (rb.fused) pack_resblock(h, rb);
    if (st.thin) pack_thin(h, st);
  }
  return HFG_OK;
}

// disc_conv (disc.h): the groups one after another, each through disc_conv_nest; f16x3 with
// the layer's exponent
int pack_disc_conv(const float* w, int cig, int cog, int k, int groups, int msub, uint16_t* dst) {
  const PackNest n = hfg::disc_conv_nest(cig, cog, k, msub);
  const size_t per = hfg::disc_conv_group_elems(cig, cog, k, msub);
  float m = 0.f;
  for (size_t i = 0; i < (size_t)groups * cog * cig * k; ++i) m = std::max(m, std::fabs(w[i]));
  const int ew = x3_exp_host(m);
  const WSplit ws{hfg::kFmtF16, std::ldexp(1.0f, ew)};
  for (int g = 0; g < groups; ++g) {
    const float* wg = w + (size_t)g * cog * cig * k;
    fill_split(n, dst + g * per, &ws, [&](const PackAt& a) {
      return a.tap < k ? wg[((size_t)a.row * cig + a.ci) * k + a.tap] : 0.f;
    });
  }
  return ew;
}

void unpack_disc_conv(const uint16_t* src, int cig, int cog, int k, int groups, int msub,
                      int plane, int ew, float* w) {
  const PackNest n = hfg::disc_conv_nest(cig, cog, k, msub);
  const size_t per = hfg::disc_conv_group_elems(cig, cog, k, msub);
  for (int g = 0; g < groups; ++g) {
    float* wg = w + (size_t)g * cog * cig * k;
    for_each_packed(n, [&](size_t i, const PackAt& a) {
      if (a.tap < k && a.plane == plane)
        wg[((size_t)a.row * cig + a.ci) * k + a.tap] = std::ldexp(h2f(src[g * per + i]), -ew);
    });
  }
}

}  // namespace hfg_host
