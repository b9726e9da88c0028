// plan.cpp — what a handle decides before any weight or input arrives: the layer list in the
// reference's order, each layer's kernel path, tile and packings, the whole-ResBlock and
// thin-stage launches with their windows and halos, the packed-buffer offsets; and the
// shapes and the workspace layout of a forward (handle.h, WsLayout).  No HIP runtime call.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <utility>

#include "handle.h"

using hfg::kTiles;
using hfg::TileCfg;

namespace hfg_host {

namespace {

// models/hifigan.py:21-23
int get_padding(int k, int d) { return (int)((k * d - d) / 2); }
// receptive-field radius of a k-tap conv at dilation d
int radius(int k, int d) { return (k - 1) / 2 * d; }
// ConvTranspose1d padding (k - u) // 2, models/hifigan.py:201 — Python floor division
int ups_padding(int k, int u) {
  int p = (k - u) / 2;
  if (k - u < 0 && (k - u) % 2 != 0) p -= 1;
  return p;
}
// (the exact-fp32 mode has no split format: -1, no scale slots)
int split_fmt(int dtype) {
  return dtype == HFG_DTYPE_BF16X3 ? hfg::kFmtBf16 : split_dtype(dtype) ? hfg::kFmtF16 : -1;
}
size_t ceil_div(size_t a, size_t b) { return (a + b - 1) / b; }

// Packed-buffer regions one after another, each 64-float aligned; len: its layout's size
// (pack_layout.h).
struct Bump {
  size_t off = 0;
  PackRegion take(size_t len) { return {std::exchange(off, off + ((len + 63) & ~(size_t)63)), len}; }
};

}  // namespace

int validate_config(const hfg_config* c) {
  if (!c) return fail(HFG_EINVAL, "config is NULL");
  if (c->n_mels <= 0) return fail(HFG_EINVAL, "n_mels must be > 0");
  if (c->n_up <= 0 || c->n_up > HFG_MAX_STAGES) return fail(HFG_EINVAL, "n_up out of range");
  if (c->n_res <= 0 || c->n_res > HFG_MAX_RES) return fail(HFG_EINVAL, "n_res out of range");
  if (c->dtype != HFG_DTYPE_FP32 && !split_dtype(c->dtype))
    return fail(HFG_EINVAL, "dtype must be HFG_DTYPE_FP32 (0), HFG_DTYPE_BF16X3 (1), "
                "HFG_DTYPE_BF16W (2) or HFG_DTYPE_F16X3 (3)");
  if (c->c0 <= 0) return fail(HFG_EINVAL, "upsample_initial_channel must be > 0");
  if (c->resblock_type != 0 && c->resblock_type != 1)
    return fail(HFG_EINVAL, "resblock_type must be 0 (the reference's ResBlock) or 1 (ResBlock2), "
                "got %d", c->resblock_type);
  // the kernels' leaky_relu is max(v, s v): s < 1
  if (!std::isfinite(c->post_slope) || c->post_slope < 0.f || c->post_slope >= 1.f)
    return fail(HFG_EINVAL, "post_slope must be finite and in [0, 1) (0 = the reference's 0.1), "
                "got %g", (double)c->post_slope);
  for (int i = 0; i < c->n_up; ++i) {
    if (c->up_rates[i] <= 0 || c->up_kernels[i] <= 0)
      return fail(HFG_EINVAL, "upsample rate/kernel %d must be > 0", i);
    if ((c->c0 >> (i + 1)) <= 0) return fail(HFG_EINVAL, "channels vanish at stage %d", i);
  }
  for (int i = 0; i < c->n_up; ++i)
    if (c->up_kernels[i] < c->up_rates[i])
      // ConvTranspose1d(padding=(k-u)//2 < 0): torch raises "negative padding is not supported"
      return fail(HFG_EINVAL, "ups.%d: kernel %d < stride %d gives negative padding (k-u)//2; "
                  "negative padding is not supported", i, c->up_kernels[i], c->up_rates[i]);
  for (int j = 0; j < c->n_res; ++j) {
    if (c->res_kernels[j] <= 0) return fail(HFG_EINVAL, "resblock kernel %d must be > 0", j);
    if (c->res_kernels[j] % 2 == 0)
      // convs2 (dilation 1, padding get_padding(k, 1) = (k-1)//2) shortens the sequence by
      // one, so the reference's residual add x + xt (models/hifigan.py:85) fails
      return fail(HFG_EINVAL, "resblock %d: even kernel size %d is not length-preserving "
                  "(the reference's residual add x + xt fails on the size mismatch)", j,
                  c->res_kernels[j]);
    if (c->n_dil[j] <= 0 || c->n_dil[j] > HFG_MAX_DIL)
      return fail(HFG_EINVAL, "resblock %d dilation count out of range", j);
    for (int m = 0; m < c->n_dil[j]; ++m)
      if (c->dil[j][m] <= 0) return fail(HFG_EINVAL, "dilation must be > 0");
  }
  return HFG_OK;
}

namespace {

void add_param(hfg_handle* h, const std::string& key, std::vector<int64_t> shape) {
  Param p;
  p.shape = std::move(shape);
  h->params[key] = std::move(p);
  h->param_order.push_back(key);
}

// A layer with weight [d0][d1][k] and bias [C_out]; its GEMM has M rows and KT taps.
int add_layer(hfg_handle* h, LayerKind kind, const std::string& mod, int cin, int cout, int k,
              int dil, int pad, int M, int KT, int64_t d0, int64_t d1) {
  Layer L{};
  L.kind = kind;
  L.mod = mod;
  L.C_in = cin;
  L.C_out = cout;
  L.k = k;
  L.dil = dil;
  L.pad = pad;
  L.M = M;
  L.KT = KT;
  h->layers.push_back(L);
  add_param(h, mod + ".weight", {d0, d1, k});
  add_param(h, mod + ".bias", {cout});
  return (int)h->layers.size() - 1;
}
int add_conv(hfg_handle* h, LayerKind kind, const std::string& mod, int cin, int cout, int k,
             int dil) {
  return add_layer(h, kind, mod, cin, cout, k, dil, get_padding(k, dil), cout, k, cout, cin);
}

// The ResBlock convs of one MRF (models/hifigan.py:96-114 / ResBlock.__init__ :34-70),
// state_dict keys "<pre>resblocks.{j}.convs{1,2}.{m}"; ResBlock2: one conv per dilation,
// "<pre>resblocks.{j}.convs.{m}" (kept in conv1).
Stage build_stage(hfg_handle* h, int ch, const std::string& pre) {
  const hfg_config& c = h->cfg;
  const bool rb2 = c.resblock_type == 1;
  Stage st;
  st.C = ch;
  for (int j = 0; j < c.n_res; ++j) {
    const int kr = c.res_kernels[j];
    const std::string rb = pre + "resblocks." + std::to_string(j);
    for (int m = 0; m < c.n_dil[j]; ++m)
      st.conv1.push_back(add_conv(h, L_CONV, rb + (rb2 ? ".convs." : ".convs1.") + std::to_string(m),
                                  ch, ch, kr, c.dil[j][m]));
    for (int m = 0; m < c.n_dil[j] && !rb2; ++m)
      st.conv2.push_back(add_conv(h, L_CONV, rb + ".convs2." + std::to_string(m), ch, ch, kr, 1));
  }
  return st;
}

// ResBlock j of stage st in execution order (conv1_0, conv2_0, conv1_1, ...; ResBlock2: its
// convs): the layer indices and each conv's receptive-field radius.
struct RbConvs {
  std::vector<int> convs, r;
  // The first conv of a launch reads its radius of x beyond the window (the kernels' spare
  // operand rows / columns) and is exact on the whole window: a launch of convs [a, b) has
  // the radii of the convs after the first as its halo.
  int halo(int a, int b) const { return std::accumulate(r.begin() + a, r.begin() + b, 0) - r[a]; }
  int r_max() const { return *std::max_element(r.begin(), r.end()); }
};
RbConvs rb_convs(const hfg_handle* h, const Stage& st, int j) {
  const hfg_config& c = h->cfg;
  int idx = 0;
  for (int q = 0; q < j; ++q) idx += c.n_dil[q];
  RbConvs rc;
  for (int m = 0; m < c.n_dil[j]; ++m, ++idx)
    for (int cv : {st.conv1[idx], c.resblock_type == 1 ? -1 : st.conv2[idx]}) {
      if (cv < 0) continue;
      rc.convs.push_back(cv);
      rc.r.push_back(radius(h->layers[cv].k, h->layers[cv].dil));
    }
  return rc;
}
// Output columns per window of nwin columns at this halo, 0 when less than nwin / 4.  A
// multiple of 4: block origins t0 = W * blockIdx stay 16-B aligned for the LDS-staged float4
// MRF epilogue (which column a block computes does not change its arithmetic: bitwise the
// same result for any W)
int window_width(int nwin, int halo) {
  const int W = (nwin - 2 * halo) & ~3;
  return W >= nwin / 4 ? W : 0;
}

// Tile, chunking and packed-buffer regions of every layer.
int plan_layers(hfg_handle* h, Bump& off) {
  for (auto& L : h->layers) {
    Packing& pk = L.pk[0];
    if (L.kind == L_POST) {
      pk.w = off.take(hfg::conv_post_pack_floats(L.C_in));
      pk.b = off.take(hfg::pack_bias_convs(1, L.C_out));
      continue;
    }
    if (split_dtype(h->cfg.dtype) && hfg::bf16x3_tile_for_rows(L.M) >= 0 &&
        hfg::bf16x3_supported(L.KT, L.dil)) {
      // split-precision path: chunk = 16 channels x TPC taps
      L.prec = 1;
      L.CK = hfg::kBf16x3Ck;
      auto packing = [&](int tile) {
        const hfg::Bf16x3Cfg& t = hfg::kBf16x3Tiles[tile];
        Packing p{tile, (int)ceil_div(L.M, t.MT()),
                  hfg::conv_bf16x3_groups(L.C_in) * hfg::conv_bf16x3_tap_groups(t, L.KT), {}, {}};
        p.w = off.take(hfg::conv_bf16x3_pack_floats(t, p.m_tiles, p.n_chunks));
        p.b = off.take(hfg::pack_bias_rows(p.m_tiles, t.MT()));
        return p;
      };
      int tile = hfg::bf16x3_tile_for_rows(L.M);
      // tile 3 with the A fragments in registers (same packing): layer convs whose tap
      // count has a compile-time instance, whole 16-channel groups
      if (tile == 3 && L.kind == L_CONV && L.C_in % 16 == 0 &&
          (L.KT == 3 || L.KT == 5 || L.KT == 7 || L.KT == 11))
        tile = h->areg_tall && L.M % hfg::kBf16x3Tiles[hfg::kAregTallTile].MT() == 0
                   ? hfg::kAregTallTile
                   : hfg::kAregTile;
      pk = packing(tile);
      if (tile != hfg::kBf16x3SmallTile && L.M >= 64) L.pk[1] = packing(hfg::kBf16x3SmallTile);
      // k = 2u upsamplers (padding u/2): the output-frame kernel's own packing
      if (L.kind == L_UPS && h->ups_frames && L.k == 2 * L.s && hfg::ups_rate_ok(L.s) &&
          L.p == L.s / 2 && L.C_in % 16 == 0) {
        // the 32-row tile (3 waves per SIMD) where the 64-row one does not divide the rows
        // (running more stages on it measured slower: two m-tiles stage one window twice)
        const int rows_f = L.C_out * L.s / 2;
        const int cfg = rows_f % hfg::kUpsCfgs[0].MT() == 0   ? 0
                        : rows_f % hfg::kUpsCfgs[1].MT() == 0 ? 1
                                                               : -1;
        if (cfg >= 0) {
          const hfg::UpsCfg& tf = hfg::kUpsCfgs[cfg];
          L.ups_cfg = cfg;
          L.m_tiles_f = rows_f / tf.MT();
          L.wf = off.take(hfg::ups_pack_floats(tf, L.m_tiles_f, L.C_in / 16));
          L.bf = off.take(hfg::pack_bias_convs(1, L.C_out));
        }
      }
      continue;
    }
    L.prec = 0;
    pk.tile = hfg::tile_for_rows(L.M);
    if (!hfg::fp32_conv_supported(pk.tile, L.KT, L.dil))
      return fail(HFG_EINVAL, "%s: %d taps at dilation %d span (k-1)*d = %d samples, beyond the "
                  "conv kernels' staging window (max %d)", L.mod.c_str(), L.KT, L.dil,
                  (L.KT - 1) * L.dil, hfg::halo_max(hfg::dispatch_kt(L.KT)));
    const TileCfg& t = kTiles[pk.tile];
    L.CK = hfg::ck_for(hfg::dispatch_kt(L.KT), pk.tile);
    pk.m_tiles = (int)ceil_div(L.M, t.MT());
    pk.n_chunks = (int)ceil_div(L.C_in, L.CK);
    pk.w = off.take(hfg::conv_f32_pack_floats(t, L.CK, L.KT, pk.m_tiles, pk.n_chunks));
    pk.b = off.take(hfg::pack_bias_rows(pk.m_tiles, t.MT()));
  }
  return HFG_OK;
}

// Whole-ResBlock launches (split precisions only): every ResBlock of the C in {32, 64}
// stages, and those of C = 128 whose receptive field costs <= 15 % recomputation (k = 3 in
// V1).  ResBlock2 (resblock2_bf16x3): one launch per block, one window per thread block (no
// split, no persistent grid, no fused conv_post).
void plan_resblocks(hfg_handle* h, Bump& off) {
  const hfg_config& c = h->cfg;
  const bool rb2 = c.resblock_type == 1;
  for (size_t i = 0; i < h->stages.size(); ++i) {
    Stage& st = h->stages[i];
    const int C = st.C;
    st.rbs.assign(c.n_res, RbFused{});
    if (!split_dtype(c.dtype) || !h->use_fused_rb || (C != 32 && C != 64 && C != 128)) continue;
    for (int j = 0; j < c.n_res; ++j) {
      const RbConvs rc = rb_convs(h, st, j);
      const int n = (int)rc.convs.size();
      RbFused rb;
      rb.convs = rc.convs;
      rb.kt = c.res_kernels[j];
      // C = 64, k = 3: a 256-column window (5 % more halo recompute than 512) whose small
      // LDS footprint lets two blocks share a CU and overlap their operand rewrites
      const int nwin = rb.nwin = C == 128 ? 256 : C == 64 ? (rb.kt == 3 ? 256 : 512) : 512;
      rb.halo = rc.halo(0, n);
      rb.W = window_width(nwin, rb.halo);
      if (rb.kt % 2 != 1 || n > hfg::kRbMaxConv || rc.r_max() > hfg::rb_marg(C, nwin) || !rb.W ||
          !(rb2 ? hfg::rb2_supported(C, rb.kt, nwin, rb.wm) : hfg::rb_supported(C, rb.kt, nwin, rb.wm)) ||
          (C == 128 && (double)nwin / rb.W > 1.15))
        continue;
      rb.fused = true;
      // the network's last MRF write: conv_post's radius 3 more halo on its last launch
      rb.post = !rb2 && h->fuse_post && h->conv_post >= 0 && i + 1 == h->stages.size() &&
                j == c.n_res - 1 && C == 32;
      const int post = rb.post ? 3 : 0;
      // two launches where that cuts the MFMA work (windows / W, weighted by the convs of
      // each part) by >= 10 %: the extra x write + read costs less than that at C <= 64
      if (h->rb_split && !rb2 && C <= 64 && c.n_dil[j] >= 2) {
        const int w_whole = window_width(nwin, rb.halo + post);
        const double whole = w_whole ? (double)nwin / w_whole : 1e9;
        double best = whole;
        for (int s = 2; s < n; s += 2) {  // between dilation pairs
          const int h0 = rc.halo(0, s), h1 = rc.halo(s, n);
          const int w0 = window_width(nwin, h0);
          const int w1p = window_width(nwin, h1 + post);  // the launch as it runs
          if (!w0 || !w1p) continue;
          const double cost = ((double)s * nwin / w0 + (double)(n - s) * nwin / w1p) / n;
          if (cost < best) {
            best = cost;
            rb.split = s;
            rb.halo_p[0] = h0;
            rb.halo_p[1] = h1;
            rb.W_p[0] = w0;
            rb.W_p[1] = window_width(nwin, h1);
          }
        }
        if (best > 0.9 * whole) rb.split = 0;
      }
      rb.halo_post = (rb.split ? rb.halo_p[1] : rb.halo) + post;
      rb.W_post = window_width(nwin, rb.halo_post);
      rb.post = rb.post && rb.halo_post >= 4 && rb.W_post;
      rb.w = off.take(hfg::rb_pack_floats(C, rb.kt, n));
      rb.b = off.take(hfg::pack_bias_convs(n, C));
      st.rbs[j] = std::move(rb);
    }
  }
}

// Thin stages (C <= 16, both precisions): one mrf_thin launch per MRF.  Each ResBlock's
// window pays the radii of all its convs.
void plan_thin(hfg_handle* h, Bump& off) {
  const hfg_config& c = h->cfg;
  for (auto& st : h->stages) {
    const int C = st.C;
    const int nwin = hfg::thin_window(C);
    // (the mrf_thin kernels compute dilation pairs only: ResBlock2 stages run layer by layer)
    if (nwin == 0 || c.n_res > hfg::kThinMaxRes || c.resblock_type == 1) continue;
    int halo_max = 0;
    bool ok = true;
    std::vector<int> convs, conv0, halos;
    for (int j = 0; j < c.n_res; ++j) {
      const RbConvs rc = rb_convs(h, st, j);
      conv0.push_back((int)convs.size());
      convs.insert(convs.end(), rc.convs.begin(), rc.convs.end());
      if (rc.r_max() > hfg::kThinMarg) ok = false;
      halos.push_back(std::accumulate(rc.r.begin(), rc.r.end(), 0));
      halo_max = std::max(halo_max, halos.back());
    }
    conv0.push_back((int)convs.size());
    const int n_conv = (int)convs.size();
    if (!ok || n_conv > hfg::kThinMaxConv || nwin - 2 * halo_max < nwin / 4) continue;
    st.thin = true;
    st.thin_convs = convs;
    st.thin_conv0 = conv0;
    st.thin_halo = halos;
    for (int cv : convs) st.thin_w.push_back(off.take(hfg::thin_pack_floats(C, h->layers[cv].k)));
    st.thin_b = off.take(hfg::pack_bias_convs(n_conv, C));
    // bf16x3: the MFMA variant when every conv's zero-padded last k-step stays in the
    // operand margin
    const int tps = 32 / C, nwin_m = hfg::thin_mfma_window(C);
    bool mf = split_dtype(c.dtype) && C == 16 && nwin_m > 0 && nwin_m - 2 * halo_max >= nwin_m / 4;
    size_t bytes = 0;
    for (int cv : convs) {
      const Layer& Lc = h->layers[cv];
      const int steps = hfg::thin_mfma_steps(C, Lc.k);
      if (((steps * tps - 1) - (Lc.k - 1) / 2) * Lc.dil > hfg::kThinMarg ||
          steps > hfg::kThinMfmaMaxSteps)
        mf = false;
      st.thin_m_conv.push_back((int)bytes);
      bytes += hfg::thin_mfma_conv_bytes(C, Lc.k);
    }
    st.thin_mfma = mf;
    if (mf) st.thin_m = off.take(hfg::pack_floats_of_bytes(bytes));
  }
}

// The layer list in the order of HiFiGANGenerator.__init__ (models/hifigan.py:177-222) (an
// MRF-only handle: the one MRF), then the plan of every launch.
int build_layers(hfg_handle* h) {
  const hfg_config& c = h->cfg;
  if (h->mrf_only) {
    h->stages.push_back(build_stage(h, c.c0 >> 1, ""));
  } else {
    h->conv_pre = add_conv(h, L_CONV, "conv_pre", c.n_mels, c.c0, 7, 1);
    std::vector<int> ups_idx;
    for (int i = 0; i < c.n_up; ++i) {
      const int cin = c.c0 >> i, cout = c.c0 >> (i + 1);
      const int u = c.up_rates[i], k = c.up_kernels[i];
      // polyphase GEMM: a row per (channel, output phase), (k + u - 1) / u taps per phase
      ups_idx.push_back(add_layer(h, L_UPS, "ups." + std::to_string(i), cin, cout, k, 1, 0, cout * u,
                                  (k + u - 1) / u, cin, cout));
      h->layers.back().s = u;
      h->layers.back().p = ups_padding(k, u);
    }
    for (int i = 0; i < c.n_up; ++i) {
      Stage st = build_stage(h, c.c0 >> (i + 1), "mrfs." + std::to_string(i) + ".");
      st.conv_ups = ups_idx[i];
      h->stages.push_back(std::move(st));
    }
    h->conv_post = add_conv(h, L_POST, "conv_post", c.c0 >> c.n_up, 1, 7, 1);
  }
  Bump off;
  const int rc = plan_layers(h, off);
  if (rc) return rc;
  plan_resblocks(h, off);
  plan_thin(h, off);
  h->packed_host.assign(off.off, 0.f);
  return HFG_OK;
}

}  // namespace

int plan_handle(hfg_handle* h) {
  // knobs of earlier rounds' schedules that no longer exist: say so instead of silently
  // running the default schedule under a variant's label
  static const char* const removed[] = {
      "HFG_SPLIT_MIN", "HFG_SPLIT_LAG", "HFG_SPLIT_STAGGER", "HFG_RB_NCH", "HFG_RB_NCH_BLOCKS",
      "HFG_UPS_SMALL_ROWS", "HFG_RB_WMR", "HFG_RB_WM", "HFG_RB_SPLIT_MIN", "HFG_RB_SPLIT_TH",
      "HFG_RB64_NARROW", "HFG_MFMA16", "HFG_EPI_LDS", "HFG_AREG", "HFG_UPS_SWIZZLE",
      "HFG_UPS_PLANES", "HFG_UPS_NT", "HFG_UPS_NT2", "HFG_THIN_MFMA", "HFG_POST4",
      "HFG_SMALL_GRID", "HFG_RB_WN32", "HFG_C16", "HFG_BF16X3_BIGTILE"};
  static std::once_flag warned;
  std::call_once(warned, [] {
    for (const char* k : removed)
      if (getenv(k))
        fprintf(stderr, "[hifigan_hip] %s is set but no longer read (a removed schedule knob); "
                        "the default schedule runs\n", k);
    // the round 1-5 environment knobs: now hfg_debug_schedule_set only
    char env[64];
    for (const SchedKnob& k : kSchedKnobs) {
      snprintf(env, sizeof(env), "HFG_%s", k.name);
      if (getenv(env))
        fprintf(stderr, "[hifigan_hip] %s is set but the library no longer reads its schedule "
                        "from the environment (hfg_debug_schedule_set); the default schedule "
                        "runs\n", env);
    }
  });
  // schedule choices the parity suites compare (each bitwise invisible, or for the fused
  // ResBlocks a different rounding order): overridden only through hfg_debug_schedule_set
#if HFG_ABLATE
  sched_apply("DEBUG_FLAGS", &h->dbg_flags);
#endif
  sched_apply("RB_PERSIST", &h->rb_persist);
  sched_apply("FUSED_RB", &h->use_fused_rb);
  sched_apply("FUSE_POST", &h->fuse_post);
  sched_apply("RB_SPLIT", &h->rb_split);
  sched_apply("SMALL_TILE", &h->small_tile);
  sched_apply("RB_CONC", &h->rb_conc);
  sched_apply("UPS_FRAMES", &h->ups_frames);
  sched_apply("SPLIT", &h->split);
  sched_apply("AREG_TALL", &h->areg_tall);
  h->fmt = split_fmt(h->cfg.dtype);
  // bf16-valued weights: their lo plane is zero, the kernels skip lo(w) * hi(x)
  if (h->cfg.dtype == HFG_DTYPE_BF16W) h->np = 2;
  return build_layers(h);
}

// ---- shape bookkeeping ------------------------------------------------------
Shapes shapes_for(const hfg_handle* h, int64_t T) {
  Shapes s;
  s.L.push_back(T);
  int64_t mx = (int64_t)h->cfg.c0 * T;
  for (int i = 0; i < h->cfg.n_up; ++i) {
    const int u = h->cfg.up_rates[i], k = h->cfg.up_kernels[i];
    const int64_t lo = (s.L.back() - 1) * u - 2 * ups_padding(k, u) + k;
    s.L.push_back(lo);
    mx = std::max(mx, (int64_t)(h->cfg.c0 >> (i + 1)) * std::max<int64_t>(lo, 0));
  }
  s.item_elems = mx;
  return s;
}

// ---- the forward workspace (handle.h, WsLayout) ------------------------------
bool stage_conc(const hfg_handle* h, const Stage& st, int64_t B, int64_t L) {
  const int n_res = h->cfg.n_res;
  if (h->rb_conc == 0 || st.thin || n_res < 2 || n_res > hfg::kMrfCombineMax) return false;
  if (h->rb_conc == 1) return true;
  return B * ((L + 255) / 256) * ((st.C + 127) / 128) < hfg_handle::kConcBlocks;
}
// small forwards stay on one stream: splitting them doubles an already latency-bound
// launch count (measured: 32 x 62 frames 5.4 -> 5.6 ms split)
bool split_batch(const hfg_handle* h, int64_t B, int64_t T) {
  return h->split >= 2 && B >= 2 && B * T >= hfg_handle::kSplitMinFrames;
}
int n_slots(const hfg_handle* h) { return (int)h->layers.size() + 2 * h->cfg.n_up + 4; }

namespace {
size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

// Regions one after another from the part's offset; every size a multiple of 256.
struct WsBump {
  size_t off;
  WsRegion take(size_t n) { return {std::exchange(off, off + align256(n)), align256(n)}; }
  WsRbRegions take_rb(size_t buf, bool out) { return {take(buf), take(buf), take(out ? buf : 0)}; }
};
// the scale slots are zeroed at the start of the forward; none in the unscaled modes
size_t slots_bytes(const hfg_handle* h, int64_t B) {
  if (h->fmt != hfg::kFmtF16) return 0;
  return (size_t)n_slots(h) * (size_t)B * hfg::kAmaxSlotWords * sizeof(uint32_t);
}

// One part of a generator forward at `off`: X, R, Tb, MRF, with concurrent ResBlocks an
// R / Tb / output triple per ResBlock, the length table, the scale slots.
WsPart part_layout(const hfg_handle* h, int64_t b0, int64_t B, int64_t T, bool conc, size_t off) {
  const Shapes sh = shapes_for(h, T);
  const size_t buf = sizeof(float) * (size_t)sh.item_elems * (size_t)B;  // one activation
  WsPart p{b0, B, off};
  WsBump at{off};
  p.X = at.take(buf);
  p.rb = at.take_rb(buf, true);
  for (size_t i = 0; conc && i < h->stages.size(); ++i)
    p.conc = p.conc || stage_conc(h, h->stages[i], B, sh.L[i + 1]);
  for (int j = 0; p.conc && j < h->cfg.n_res; ++j) p.rb_conc[j] = at.take_rb(buf, true);
  p.table = at.take((size_t)(h->cfg.n_up + 1) * (size_t)B * sizeof(int32_t));
  p.slots = at.take(slots_bytes(h, B));
  p.bytes = at.off - off;
  return p;
}
}  // namespace

// Both halves when the batch is split over two streams (whose ResBlocks then run one after
// another), else one part with concurrent ResBlocks allowed.
WsLayout ws_layout(const hfg_handle* h, int64_t B, int64_t T, bool taps) {
  const bool split = split_batch(h, B, T);
  const int64_t B1 = split && !taps ? (B + 1) / 2 : B;
  WsLayout w;
  w.part[0] = part_layout(h, 0, B1, T, !split, 0);
  w.total = w.part[0].bytes;
  if (B1 < B) {
    w.n_parts = 2;
    w.part[1] = part_layout(h, B1, B - B1, T, false, w.total);
    w.total += w.part[1].bytes;
  }
  return w;
}
// (the taps layout never is the larger one, every term of a part being subadditive in B;
// taking the max states that instead of relying on it)
size_t ws_bytes_for(const hfg_handle* h, int64_t B, int64_t T) {
  return std::max(ws_layout(h, B, T, false).total, ws_layout(h, B, T, true).total);
}
// R and Tb of the layer-per-launch ResBlocks ([B][C][L] each), the scale slots
WsLayout mrf_ws_layout(const hfg_handle* h, int64_t B, int64_t L) {
  WsLayout w;
  WsPart& p = w.part[0];
  p.B = B;
  WsBump at{0};
  p.rb = at.take_rb(sizeof(float) * (size_t)B * h->stages[0].C * (size_t)L, false);
  p.slots = at.take(slots_bytes(h, B));
  w.total = p.bytes = at.off;
  return w;
}

}  // namespace hfg_host
