// pack.cpp — the handle's weights in the operand orders the kernels read: weight-norm
// folded fp32 tensors -> h->packed_host at the offsets of the plan (plan.cpp).  Host only.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "handle.h"

using hfg::kTiles;
using hfg::TileCfg;

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

// mrf_thin weights: per conv [tap][ci][co] fp32 (the C output channels of one (tap, ci)
// are one scalar load), biases [conv][C]
void pack_thin(hfg_handle* h, const Stage& st) {
  const int C = st.C;
  for (size_t e = 0; e < st.thin_convs.size(); ++e) {
    const Layer& L = h->layers[st.thin_convs[e]];
    const float* w = weight_of(h, L);  // [C_out][C_in][k]
    float* dst = h->packed_host.data() + st.thin_w_off[e];
    for (int j = 0; j < L.k; ++j)
      for (int ci = 0; ci < C; ++ci)
        for (int co = 0; co < C; ++co)
          dst[((size_t)j * C + ci) * C + co] = w[((size_t)co * C + ci) * L.k + j];
    std::copy_n(bias_of(h, L), C, h->packed_host.data() + st.thin_b_off + e * C);
  }
  if (!st.thin_mfma) return;
  // mrf_thin_mfma A stream (C = 16): per (conv, k-step) [plane][lane][8], lane l -> row
  // r = l & 15, ci = 8 ((l >> 4) & 1) + e, tap = 2 s + (l >> 5); plane 0 = hi, 1 = lo
  const int tps = 32 / C;
  for (size_t e = 0; e < st.thin_convs.size(); ++e) {
    const Layer& L = h->layers[st.thin_convs[e]];
    const WSplit ws = wsplit(h, L);
    const float* w = weight_of(h, L);  // [C_out][C_in][k]
    const int steps = (L.k + tps - 1) / tps;
    uint16_t* de = halves_at(h, st.thin_m_off) + st.thin_m_conv[e] / 2;
    for (int s = 0; s < steps; ++s)
      for (int plane = 0; plane < 2; ++plane)
        for (int lane = 0; lane < 64; ++lane)
          for (int el = 0; el < 8; ++el) {
            const int co = lane & 15, qq = lane >> 4;
            const int ci = 8 * (qq & 1) + el, tap = 2 * s + (qq >> 1);
            const float v = tap < L.k ? w[((size_t)co * C + ci) * L.k + tap] : 0.f;
            de[((size_t)(s * 2 + plane) * 64 + lane) * 8 + el] = split_w(v, ws, plane);
          }
  }
}

// Fragment order of conv1d_mfma_f32's A operand (see conv_kernels.hip):
//   idx = ((((mt*n_chunks + c)*KT + j)*KK + kk)*WAVES_M + wave_m)*64*WM + lane*WM + wm
//   row = mt*MT + wave_m*32*WM + wm*32 + (lane & 31),  ci = c*CK + 2*kk + (lane >> 5)
// wt(row, ci, j) is the GEMM weight; zero outside [0,M) x [0,C_in).
template <typename F>
void pack_gemm_weights(const Layer& L, const Packing& pk, F wt, float* dst) {
  const TileCfg& t = kTiles[pk.tile];
  const int KK = L.CK / 2;
  size_t idx = 0;
  for (int mt = 0; mt < pk.m_tiles; ++mt)
    for (int c = 0; c < pk.n_chunks; ++c)
      for (int j = 0; j < L.KT; ++j)
        for (int kk = 0; kk < KK; ++kk)
          for (int wave_m = 0; wave_m < t.WAVES_M; ++wave_m)
            for (int lane = 0; lane < 64; ++lane)
              for (int wm = 0; wm < t.WM; ++wm) {
                const int row = mt * t.MT() + wave_m * 32 * t.WM + wm * 32 + (lane & 31);
                const int ci = c * L.CK + 2 * kk + (lane >> 5);
                dst[idx++] = (row < L.M && ci < L.C_in) ? wt(row, ci, j) : 0.f;
              }
}

// A-fragment order of conv1d_bf16x3 (conv_bf16x3.hip), in bf16 elements:
//   idx = ((((((mt*n_g + g)*n_tg + tg)*TPC + jj)*2 + plane)*WAVES_M + wave_m)*WM + wm)*512
//         + lane*8 + e
//   row = mt*MT + wave_m*32*WM + wm*32 + (lane & 31), ci = g*16 + 8*(lane >> 5) + e,
//   tap = tg*TPC + jj; plane 0 = bf16(w), plane 1 = bf16(w - hi).
template <typename F>
void pack_bf16x3(const Layer& L, const Packing& pk, F wt, const WSplit& ws, uint16_t* dst) {
  const hfg::Bf16x3Cfg& t = hfg::kBf16x3Tiles[pk.tile];
  const int TPC = t.TPC;
  const int n_g = (L.C_in + 15) / 16, n_tg = (L.KT + TPC - 1) / TPC;
  size_t idx = 0;
  for (int mt = 0; mt < pk.m_tiles; ++mt)
    for (int g = 0; g < n_g; ++g)
      for (int tg = 0; tg < n_tg; ++tg)
        for (int jj = 0; jj < TPC; ++jj)
          for (int plane = 0; plane < 2; ++plane)
            for (int wave_m = 0; wave_m < t.WAVES_M; ++wave_m)
              for (int wm = 0; wm < t.WM; ++wm)
                for (int lane = 0; lane < 64; ++lane)
                  for (int e = 0; e < 8; ++e) {
                    const int row = mt * t.MT() + wave_m * 32 * t.WM + wm * 32 + (lane & 31);
                    const int ci = g * 16 + 8 * (lane >> 5) + e;
                    const int tap = tg * TPC + jj;
                    float v = 0.f;
                    if (row < L.M && ci < L.C_in && tap < L.KT) v = wt(row, ci, tap);
                    dst[idx++] = split_w(v, ws, plane);
                  }
}

// A stream of resblock_bf16x3 (resblock_bf16x3.hip), in bf16 elements:
//   idx = (((((wave_m*n_conv + e)*n_g + g)*KT + tap)*2 + plane)*64 + lane)*8 + el
//   row = wave_m*32 + (lane & 31), ci = g*16 + 4*(lane >> 5) + (el & 3) + 8*(el >> 2)
// (the permuted channel order of the kernel's operand planes); plane 0 = bf16(w),
// plane 1 = bf16(w - hi).  Biases [conv][C].
void pack_resblock(hfg_handle* h, const RbFused& rb) {
  uint16_t* dst = halves_at(h, rb.w_off);
  const int n_conv = (int)rb.convs.size();
  const int C = h->layers[rb.convs[0]].C_out;
  const int KT = rb.kt, n_g = C / 16;
  size_t idx = 0;
  for (int wm = 0; wm < C / 32; ++wm)
    for (int e = 0; e < n_conv; ++e) {
      const Layer& L = h->layers[rb.convs[e]];
      const WSplit ws = wsplit(h, L);
      const float* w = weight_of(h, L);  // [C_out][C_in][k]
      for (int g = 0; g < n_g; ++g)
        for (int tap = 0; tap < KT; ++tap)
          for (int plane = 0; plane < 2; ++plane)
            for (int lane = 0; lane < 64; ++lane)
              for (int el = 0; el < 8; ++el) {
                const int row = wm * 32 + (lane & 31);
                const int ci = g * 16 + 4 * (lane >> 5) + (el & 3) + 8 * (el >> 2);
                dst[idx++] = split_w(w[((size_t)row * C + ci) * KT + tap], ws, plane);
              }
    }
  for (int e = 0; e < n_conv; ++e)
    std::copy_n(bias_of(h, h->layers[rb.convs[e]]), C,
                h->packed_host.data() + rb.b_off + (size_t)e * C);
}

// A slabs of ups_bf16x3 (ups_bf16x3.hip), in bf16 elements:
//   idx = (((((((mt*n_g + g)*2 + c)*2 + tp)*2 + plane)*WAVES_M + wave_m)*WM + wm)*64 + lane)*8 + e
//   class row rr = mt*MT + wave_m*32*WM + wm*32 + (lane & 31) -> co = rr / h, s' = rr % h
//   (h = u/2), ci = g*16 + 8*(lane >> 5) + e; kernel index (nn.ConvTranspose1d weight
//   [C_in][C_out][k]): class L (c = 0) tap 0 (x[m-1]) s'+h+u, tap 1 (x[m]) s'+h;
//   class R (c = 1) tap 0 (x[m]) s'+u, tap 1 (x[m+1]) s'.  Bias [C_out].
void pack_ups_frames(hfg_handle* h, const Layer& L) {
  const hfg::UpsCfg& t = hfg::kUpsCfgs[L.ups_cfg];
  const float* w = weight_of(h, L);
  uint16_t* dst = halves_at(h, L.wf_off);
  const WSplit ws = wsplit(h, L);
  const int u = L.s, hh = u / 2, k = L.k, cout = L.C_out, n_g = L.C_in / 16;
  size_t idx = 0;
  for (int mt = 0; mt < L.m_tiles_f; ++mt)
    for (int g = 0; g < n_g; ++g)
      for (int c = 0; c < 2; ++c)
        for (int tp = 0; tp < 2; ++tp)
          for (int plane = 0; plane < 2; ++plane)
            for (int wave_m = 0; wave_m < t.WAVES_M; ++wave_m)
              for (int wm = 0; wm < t.WM; ++wm)
                for (int lane = 0; lane < 64; ++lane)
                  for (int e = 0; e < 8; ++e) {
                    const int rr = mt * t.MT() + wave_m * 32 * t.WM + wm * 32 + (lane & 31);
                    const int co = rr / hh, sp = rr % hh;
                    const int ci = g * 16 + 8 * (lane >> 5) + e;
                    const int j = c == 0 ? (tp == 0 ? sp + hh + u : sp + hh) : (tp == 0 ? sp + u : sp);
                    dst[idx++] = split_w(w[((size_t)ci * cout + co) * k + j], ws, plane);
                  }
  std::copy_n(bias_of(h, L), cout, h->packed_host.data() + L.bf_off);
}

void pack_layer(hfg_handle* h, const Layer& L) {
  const float* w = weight_of(h, L);
  const float* bias = bias_of(h, L);
  float* packed = h->packed_host.data();
  if (L.kind == L_POST) {
    std::memcpy(packed + L.pk[0].w_off, w, sizeof(float) * L.C_in * 7);  // [1][C][7]
    packed[L.pk[0].b_off] = bias[0];
    return;
  }
  // The GEMM weight wt(row, ci, tap).  Conv1d: nn.Conv1d weight [C_out][C_in][k].  Polyphase
  // ConvTranspose1d: row m = co*s + r; tap jj reads x[u - (Q-1) + jj], i.e. original kernel
  // index r + s*(Q-1-jj) of the nn.ConvTranspose1d weight [C_in][C_out][k].
  const int cin = L.C_in, cout = L.C_out, k = L.k, s = L.kind == L_UPS ? L.s : 1, Q = L.KT;
  auto wt = [&](int row, int ci, int jj) {
    if (L.kind == L_CONV) return w[((size_t)row * cin + ci) * k + jj];
    const int co = row / s, r = row % s;
    const int kidx = r + s * (Q - 1 - jj);
    return kidx < k ? w[((size_t)ci * cout + co) * k + kidx] : 0.f;
  };
  // the layer's tile, then (split-precision layers with one) the small-grid tile
  for (const Packing& pk : L.pk) {
    if (pk.tile < 0) continue;
    if (L.prec == 1)
      pack_bf16x3(L, pk, wt, wsplit(h, L), halves_at(h, pk.w_off));
    else
      pack_gemm_weights(L, pk, wt, packed + pk.w_off);
    for (size_t m = 0; m < pk.b_len; ++m) packed[pk.b_off + m] = m < (size_t)L.M ? bias[m / s] : 0.f;
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

}  // namespace hfg_host
