// forward.cpp — the launch schedule of HiFiGANGenerator.forward (models/hifigan.py:224-261)
// on a committed handle: conv_pre, per stage the upsampler and the MRF (whole-ResBlock, thin
// or layer-by-layer launches, one after another or concurrent), conv_post; the two-stream
// batch split; the MRF-only forwards; the weight upload of a commit.
#include <algorithm>
#include <set>

#include "handle.h"

using hfg::ConvParams;
using hfg::kTiles;
using hfg::TileId;

namespace hfg {
std::mutex& setup_mutex() {
  static std::mutex mu;
  return mu;
}
hipError_t ensure_max_lds(const void* fn) {
  static std::set<std::pair<const void*, int>> done;
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  std::lock_guard<std::mutex> lk(setup_mutex());
  if (done.count({fn, dev})) return hipSuccess;
  e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLdsBytes);
  if (e == hipSuccess) done.insert({fn, dev});
  return e;
}
}  // namespace hfg

namespace hfg_host {

int do_commit(hfg_handle* h) {
  int rc = pack_weights(h);
  if (rc) return rc;
  if (h->device >= 0) {
    DeviceGuard g(h->device);
    if (!g.ok) return fail(HFG_ENODEV, "hipSetDevice(%d) failed", h->device);
    // a previous forward may still read the old weights
    hipError_t se = hipDeviceSynchronize();
    if (se != hipSuccess) return hip_fail(se, "hipDeviceSynchronize(commit)");
    if (h->packed_dev_len < h->packed_host.size()) {
      if (h->packed_dev) (void)hipFree(h->packed_dev);
      h->packed_dev = nullptr;
      h->packed_dev_len = 0;
      hipError_t e = hipMalloc(&h->packed_dev, sizeof(float) * h->packed_host.size());
      if (e != hipSuccess) return fail(HFG_ENOMEM, "hipMalloc(weights): %s", hipGetErrorString(e));
      h->packed_dev_len = h->packed_host.size();
    }
    hipError_t e = hipMemcpy(h->packed_dev, h->packed_host.data(),
                             sizeof(float) * h->packed_host.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) return hip_fail(e, "hipMemcpy(weights)");
  }
  h->dirty = false;
  return HFG_OK;
}

void recycle_prof(hfg_handle* h) {
  for (auto& r : h->prof) {
    if (r.e0) h->event_pool.push_back(r.e0);
    if (r.e1) h->event_pool.push_back(r.e1);
  }
  h->prof.clear();
}

namespace {

hipEvent_t pool_event(hfg_handle* h) {
  if (!h->event_pool.empty()) {
    hipEvent_t e = h->event_pool.back();
    h->event_pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  if (hipEventCreate(&e) != hipSuccess) return nullptr;
  return e;
}

// f16x3 activation scales of one forward part (bf16x3_common.h): slot rows handed out in
// launch order; base null in the unscaled modes (every take() is then null)
struct Slots {
  uint32_t* base = nullptr;
  int n = 0, next = 0;
  int64_t B = 0;
  bool overflow = false;
  // f16x3: the slots at `at` (slots_bytes(h, B) of the workspace), zeroed on the stream
  int begin(const hfg_handle* h, void* at, int64_t batch, hipStream_t stream) {
    if (h->fmt != hfg::kFmtF16) return HFG_OK;
    base = static_cast<uint32_t*>(at);
    n = n_slots(h);
    B = batch;
    hipError_t e = hipMemsetAsync(base, 0, slots_bytes(h, B), stream);
    return e == hipSuccess ? HFG_OK : hip_fail(e, "hipMemsetAsync(scale slots)");
  }
  uint32_t* take() {
    if (!base) return nullptr;
    if (next >= n) {  // sized by n_slots(): a schedule that needs more is a bug
      overflow = true;
      return nullptr;
    }
    return base + (size_t)(next++) * (size_t)B * hfg::kAmaxSlotWords;
  }
  int end() const {
    return overflow ? fail(HFG_EIO, "internal: f16x3 scale slots exhausted") : HFG_OK;
  }
};

struct Launcher {
  hfg_handle* h;
  hipStream_t stream;
  int part = 0;
  int seq = 0;
  int conc = 1;  // launches of this schedule running side by side (concurrent ResBlocks)
  Slots* sl = nullptr;
  ProfRec* rec = nullptr;
  uint32_t* take() { return sl ? sl->take() : nullptr; }
  void begin(double flop, double bytes) {
    rec = nullptr;
    if (!h->profiling) return;
    ProfRec r{nullptr, flop, bytes, pool_event(h), pool_event(h), h->fwd_count, part, seq++};
    if (r.e0) (void)hipEventRecord(r.e0, stream);
    h->prof.push_back(r);
    rec = &h->prof.back();
  }
  void end(const char* label) {
    if (!rec) return;
    rec->label = label;
    if (rec->e1) (void)hipEventRecord(rec->e1, stream);
  }
};

// What a Conv1d and a polyphase ConvTranspose1d launch share: x [B][C_in][Lin] ->
// y [B][C_out][Lout] as a GEMM of L.M rows x L.KT taps.
// ain / aout: f16x3 scale slots of the input (its producer's) and of this launch's output
ConvParams layer_params(const hfg_handle* h, const Layer& L, const float* x, int64_t Lin, float* y,
                        int64_t Lout, const int32_t* len_in, const int32_t* len_out,
                        const uint32_t* ain, uint32_t* aout) {
  ConvParams p{};
  p.x = x;
  p.x_bs = (int64_t)L.C_in * Lin;
  p.x_cs = Lin;
  p.x_ts = 1;
  p.C_in = L.C_in;
  p.L_in = (int)Lin;
  p.len_in = len_in;
  p.len_out = len_out;
  p.y = y;
  p.y_bs = (int64_t)L.C_out * Lout;
  p.M = L.M;
  p.dil = L.dil;
  p.kt = L.KT;
  p.amax_in = ain;
  p.amax_out = aout;
  p.ew = L.ew;
  p.dbg = h->dbg_flags;
  return p;
}

// The launch of a layer whose p.N output columns are set: the packing (a split-precision
// layer whose own tile would leave most CUs idle, fewer than kSmallGridBlocks blocks over
// the `conc` launches that share the chip, runs the small tile on its own packing: bitwise
// the same result, kernels.h tile 4), the profile record, the kernel of the layer's precision.
int launch_layer(hfg_handle* h, Launcher& ln, const Layer& L, ConvParams& p, bool ups, int64_t B,
                 double flop, double bytes) {
  auto n_tiles_of = [&](const Packing& pk) {
    const int nt = L.prec == 1 ? hfg::kBf16x3Tiles[pk.tile].NTILE() : kTiles[pk.tile].NTILE();
    return (p.N + nt - 1) / nt;
  };
  const Packing* pk = &L.pk[0];
  if (L.prec == 1 && L.pk[1].tile >= 0 &&
      (h->small_tile == 1 ||
       (h->small_tile != 0 &&
        (int64_t)n_tiles_of(*pk) * pk->m_tiles * B * ln.conc < hfg::kSmallGridBlocks)))
    pk = &L.pk[1];
  p.w = h->packed_dev + pk->w_off;
  p.bias = h->packed_dev + pk->b_off;
  p.n_chunks = pk->n_chunks;
  const char* name = nullptr;
  ln.begin(flop, bytes);
  hipError_t e = L.prec == 1
                     ? hfg::launch_conv_bf16x3(pk->tile, L.KT, ups, h->fmt, h->np, p, n_tiles_of(*pk),
                                               pk->m_tiles, (int)B, ln.stream, &name)
                     : hfg::launch_conv((TileId)pk->tile, L.KT, ups, p, n_tiles_of(*pk), pk->m_tiles,
                                        (int)B, ln.stream, &name);
  ln.end(name);
  if (e != hipSuccess) return fail(HFG_EIO, "launch %s: %s", L.mod.c_str(), hipGetErrorString(e));
  return HFG_OK;
}

// One conv-layer launch (regular Conv1d).
int run_conv(hfg_handle* h, Launcher& ln, const Layer& L, const float* x, int64_t B, int64_t Lt,
             float* y, bool act_in, bool act_out, const float* res, float* mrf, int mrf_mode,
             float mrf_div, const int32_t* lens, const uint32_t* ain, uint32_t* aout,
             bool x_btc = false) {
  ConvParams p = layer_params(h, L, x, Lt, y, Lt, lens, lens, ain, aout);
  if (x_btc) {  // [B][T][C] (acoustic-model layout) instead of [B][C][T]
    p.x_cs = 1;
    p.x_ts = L.C_in;
  }
  p.N = (int)Lt;
  p.off = -L.pad;
  p.act_in = act_in;
  p.act_out = act_out;
  p.res = res;
  p.mrf = mrf;
  p.mrf_mode = mrf_mode;
  p.mrf_div = mrf_div;
  p.epi_lds = 1;
  const double flop = 2.0 * L.C_out * L.C_in * L.k * (double)Lt * B;
  double bytes = 4.0 * B * Lt * (L.C_in + L.C_out) + 4.0 * L.C_out * L.C_in * L.k;
  if (res) bytes += 4.0 * B * Lt * L.C_out;
  if (mrf && (mrf_mode & 1)) bytes += 4.0 * B * Lt * L.C_out;
  return launch_layer(h, ln, L, p, false, B, flop, bytes);
}

// slope of the leaky_relu in front of conv_post: the reference's 0.1 (models/hifigan.py:254)
// unless the config names another (the public release's F.leaky_relu(x) default, 0.01)
inline float post_slope_of(const hfg_handle* h) {
  return h->cfg.post_slope ? h->cfg.post_slope : hfg::kLReluSlope;
}

struct PostFuse {
  const float* w;  // conv_post weight [C][7], bias [1] (packed fp32)
  const float* b;
  float* wav;      // [B][L]
  float slope;     // of the leaky_relu in front of conv_post (post_slope_of)
};

// One whole ResBlock (all dilations) + its MRF contribution in one launch.
// A split ResBlock (rb.split) runs as two launches through `scratch` (B*C*L floats): convs
// [0, split) write x after their dilation pairs (MRF-epilogue mode 0: a plain store), convs
// [split, n) read it back and do the MRF epilogue.  fp32 round trip: bitwise the same x.
// post: conv_post + tanh fused into the last launch (C = 32, the network's last MRF write).
int run_resblock(hfg_handle* h, Launcher& ln, const RbFused& rb, const float* x, int64_t B,
                 int64_t Lt, float* mrf, int mrf_mode, float mrf_div, const int32_t* lens,
                 float* scratch, uint32_t* aout, const PostFuse* post = nullptr) {
  const Layer& L0 = h->layers[rb.convs[0]];
  const int C = L0.C_out;
  const int n_all = (int)rb.convs.size();
  const int n_part = rb.split && scratch ? 2 : 1;
  for (int part = 0; part < n_part; ++part) {
    const int c0 = n_part == 1 ? 0 : (part == 0 ? 0 : rb.split);
    const int c1 = n_part == 1 ? n_all : (part == 0 ? rb.split : n_all);
    const bool last = part == n_part - 1;
    hfg::RbParams p{};
    p.x = part == 0 ? x : scratch;
    p.bs = (int64_t)C * Lt;
    p.L = (int)Lt;
    p.len = lens;
    p.w = reinterpret_cast<const __bf16*>(h->packed_dev + rb.w_off);
    p.w_bytes = (int)(rb.w_len * sizeof(float));
    p.bias = h->packed_dev + rb.b_off + (size_t)c0 * C;
    p.n_conv = c1 - c0;
    p.conv0 = c0;
    p.n_conv_stream = n_all;
    double flop = 0.0;
    for (int e = c0; e < c1; ++e) {
      const Layer& L = h->layers[rb.convs[e]];
      p.dil[e - c0] = L.dil;
      p.ew[e - c0] = L.ew;
      flop += 2.0 * L.C_out * L.C_in * L.k * (double)Lt * B;
    }
    p.halo = n_part == 1 ? rb.halo : rb.halo_p[part];
    p.W = n_part == 1 ? rb.W : rb.W_p[part];
    p.mrf = last ? mrf : scratch;
    p.mrf_mode = last ? mrf_mode : 0;
    p.mrf_div = mrf_div;
    p.mrf_rcp = hfg::fast_div_ok(mrf_div) ? 1.0f / mrf_div : 0.0f;
    p.amax_out = last ? aout : nullptr;
    p.dbg = h->dbg_flags;
    // resident blocks per CU from the LDS footprint
    const int per_cu = hfg::rb_lds_bytes(C, rb.nwin, n_all) <= hfg::kMaxLdsBytes / 2 ? 2 : 1;
    // a persistent grid of the resident blocks (each window's x load overlaps the previous
    // window's MRF round trip; launch_resblock_bf16x3 runs it where a persistent variant is
    // built, C = 64 with the 512-column window).  RB_PERSIST: 0 off, 1 one block per CU
    // of the half-batch stream's share (n_CU / halves), 2 one per CU
    const bool rb2 = h->cfg.resblock_type == 1;  // resblock2_bf16x3: one window per block
    if (h->rb_persist && per_cu == 1 && !(last && post) && !rb2)
      p.persist = std::max(1, h->n_cu / (h->rb_persist == 1 ? h->halves : 1));
    double bytes =
        4.0 * B * Lt * C * ((last && (mrf_mode & 1)) ? 3 : 2) + 4.0 * (double)rb.w_len;
    if (last && post) {
      // the stage output is exact on the centre plus conv_post's radius on either side
      p.halo = rb.halo_post;
      p.W = rb.W_post;
      p.post_w = post->w;
      p.post_b = post->b;
      p.post_slope = post->slope;
      p.wav = post->wav;
      p.amax_out = nullptr;  // no consumer of the stage output's scale
      bytes -= 4.0 * B * Lt * (C - 1);
    }
    const char* name = nullptr;
    ln.begin(flop, bytes);
    hipError_t e =
        rb2 ? hfg::launch_resblock2_bf16x3(C, rb.nwin, rb.wm, rb.kt, h->fmt, h->np, p, (int)B,
                                           ln.stream, &name)
            : hfg::launch_resblock_bf16x3(C, rb.nwin, rb.wm, rb.kt, h->fmt, h->np, p, (int)B,
                                          ln.stream, &name);
    ln.end(name);
    if (e != hipSuccess)
      return fail(HFG_EIO, "launch resblock %s: %s", L0.mod.c_str(), hipGetErrorString(e));
  }
  return HFG_OK;
}

int run_ups(hfg_handle* h, Launcher& ln, const Layer& L, const float* x, int64_t B, int64_t Lin,
            int64_t Lout, float* y, const int32_t* len_in, const int32_t* len_out,
            const uint32_t* ain, uint32_t* aout) {
  const double flop = 2.0 * L.C_in * L.C_out * L.k * (double)Lin * B;
  const double bytes = 4.0 * B * (L.C_in * Lin + L.C_out * Lout) + 4.0 * L.C_in * L.C_out * L.k;
  if (L.ups_cfg >= 0 && h->ups_frames && Lin % 4 == 0 && Lout == Lin * L.s) {
    // output-frame kernel, unless its grid would leave most CUs idle (then the polyphase
    // kernel's small-grid tile): bitwise the same result either way
    const int cfg = L.ups_cfg;
    const hfg::UpsCfg& t = hfg::kUpsCfgs[cfg];
    const int n_tiles = (int)((Lin + t.NTILE() - 1) / t.NTILE());
    if (h->ups_frames == 2 ||
        (int64_t)L.m_tiles_f * n_tiles * B * ln.conc >= hfg::kSmallGridBlocks) {
      hfg::UpsParams q{};
      q.x = x;
      q.x_bs = (int64_t)L.C_in * Lin;
      q.C_in = L.C_in;
      q.L = (int)Lin;
      q.T = (int)Lin;
      q.len_in = len_in;
      q.w = reinterpret_cast<const __bf16*>(h->packed_dev + L.wf_off);
      q.bias = h->packed_dev + L.bf_off;
      q.y = y;
      q.y_bs = (int64_t)L.C_out * Lout;
      q.C_out = L.C_out;
      q.L_out = (int)Lout;
      q.u = L.s;
      q.m_tiles = L.m_tiles_f;
      q.n_tiles = n_tiles;
      q.batch = (int)B;
      q.amax_in = ain;
      q.amax_out = aout;
      q.ew = L.ew;
      q.dbg = h->dbg_flags;
      const char* name = nullptr;
      ln.begin(flop, bytes);
      hipError_t e = hfg::launch_ups_bf16x3(cfg, h->fmt, h->np, q, ln.stream, &name);
      ln.end(name);
      if (e != hipSuccess)
        return fail(HFG_EIO, "launch %s: %s", L.mod.c_str(), hipGetErrorString(e));
      return HFG_OK;
    }
  }
  ConvParams p = layer_params(h, L, x, Lin, y, Lout, len_in, len_out, ain, aout);
  // columns u: t_out + p = s*u + r  for t_out in [0, Lout)
  p.N = (int)((Lout - 1 + L.p) / L.s + 1);
  p.off = -(L.KT - 1);
  p.act_in = 1;  // F.leaky_relu before every upsample, models/hifigan.py:244
  p.ups_s = L.s;
  p.ups_p = L.p;
  p.ups_swz = 1;
  p.L_out = (int)Lout;
  return launch_layer(h, ln, L, p, true, B, flop, bytes);
}

// A thin stage's whole MRF (or ResBlock only_j alone) in one mrf_thin launch.
int run_thin(hfg_handle* h, Launcher& ln, const Stage& st, const float* X, int64_t B, int64_t Lt,
             float* out, const int32_t* lens, int only_j, uint32_t* aout) {
  const hfg_config& c = h->cfg;
  const int C = st.C;
  hfg::ThinParams p{};
  p.x = X;
  p.bs = (int64_t)C * Lt;
  p.L = (int)Lt;
  p.len = lens;
  p.w = h->packed_dev;
  const int j0 = only_j >= 0 ? only_j : 0, j1 = only_j >= 0 ? only_j + 1 : c.n_res;
  p.n_res = j1 - j0;
  const int cv_base = st.thin_conv0[j0];
  double flop = 0.0, wbytes = 0.0;
  int halo = 0;
  for (int j = j0; j < j1; ++j) {
    p.rb_conv0[j - j0] = st.thin_conv0[j] - cv_base;
    halo = std::max(halo, st.thin_halo[j]);
  }
  p.rb_conv0[p.n_res] = st.thin_conv0[j1] - cv_base;
  for (int e = st.thin_conv0[j0]; e < st.thin_conv0[j1]; ++e) {
    const Layer& L = h->layers[st.thin_convs[e]];
    const int q = e - cv_base;
    p.kt[q] = L.k;
    p.dil[q] = L.dil;
    p.ew[q] = L.ew;
    p.w_off[q] = (int)st.thin_w_off[e];
    flop += 2.0 * C * C * L.k * (double)Lt * B;
    wbytes += 4.0 * C * C * L.k;
  }
  // the kernel indexes biases as [conv][C] from this launch's first conv
  p.bias = h->packed_dev + st.thin_b_off + (size_t)cv_base * C;
  p.halo = halo;
  p.W = (st.thin_mfma ? hfg::thin_mfma_window(C) : hfg::thin_window(C)) - 2 * halo;
  p.y = out;
  p.div = (float)p.n_res;
  p.amax_out = aout;
  if (st.thin_mfma) {
    const int base = st.thin_m_conv[cv_base];
    p.wm = reinterpret_cast<const __bf16*>(h->packed_dev + st.thin_m_off) + base / 2;
    p.wm_bytes = (int)st.thin_m_bytes - base;
    for (int e = st.thin_conv0[j0]; e < st.thin_conv0[j1]; ++e)
      p.wm_off[e - cv_base] = st.thin_m_conv[e] - base;
  }
  const double bytes = 8.0 * B * Lt * C + wbytes;  // x once, y once, weights once
  const char* name = nullptr;
  ln.begin(flop, bytes);
  hipError_t e = st.thin_mfma ? hfg::launch_mrf_thin_mfma(C, h->fmt, h->np, p, (int)B, ln.stream, &name)
                               : hfg::launch_mrf_thin(C, p, (int)B, ln.stream, &name);
  ln.end(name);
  if (e != hipSuccess) return fail(HFG_EIO, "launch mrf_thin (C=%d): %s", C, hipGetErrorString(e));
  return HFG_OK;
}

// ResBlock j of stage st (ResBlock.forward, models/hifigan.py:72-86) on X, its result
// combined into out by the MRF epilogue mode (bit0 add, bit1 divide by n_res); idx = index
// of its first dilation in st.conv1 / st.conv2.  R, Tb: scratch of the layer-per-launch path.
// f16x3: ax = scale slot of X; aout = slot of out (committed by the write that completes it)
int run_one_rb(hfg_handle* h, Launcher& ln, const Stage& st, int j, int idx, const float* X,
               int64_t B, int64_t L, float* R, float* Tb, float* out, int mode,
               const int32_t* lens, const uint32_t* ax, uint32_t* aout,
               const PostFuse* post = nullptr) {
  const hfg_config& c = h->cfg;
  if (st.rbs[j].fused)
    return run_resblock(h, ln, st.rbs[j], X, B, L, out, mode, (float)c.n_res, lens, Tb, aout,
                        post);
  int rc;
  const uint32_t* asrc = ax;
  if (c.resblock_type == 1) {
    // ResBlock2, one launch per dilation: x = x + conv_m(lrelu(x)).  The conv reads a
    // neighbourhood of x, so it writes the other of R / Tb; the last one carries the MRF epilogue
    const float* src = X;
    for (int m = 0; m < c.n_dil[j]; ++m, ++idx) {
      const Layer& Lm = h->layers[st.conv1[idx]];
      if (m < c.n_dil[j] - 1) {
        float* dst = (m & 1) ? Tb : R;
        uint32_t* ar = ln.take();
        rc = run_conv(h, ln, Lm, src, B, L, dst, true, false, src, nullptr, 0, 1.f, lens, asrc, ar);
        src = dst;
        asrc = ar;
      } else {
        rc = run_conv(h, ln, Lm, src, B, L, nullptr, true, false, src, out, mode, (float)c.n_res,
                      lens, asrc, aout);
      }
      if (rc) return rc;
    }
    return HFG_OK;
  }
  for (int m = 0; m < c.n_dil[j]; ++m, ++idx) {
    const float* src = (m == 0) ? X : R;
    const Layer& L1 = h->layers[st.conv1[idx]];
    const Layer& L2 = h->layers[st.conv2[idx]];
    // xt = lrelu(conv1(lrelu(x)))
    uint32_t* at = ln.take();
    rc = run_conv(h, ln, L1, src, B, L, Tb, true, true, nullptr, nullptr, 0, 1.f, lens, asrc, at);
    if (rc) return rc;
    if (m < c.n_dil[j] - 1) {
      // x = x + conv2(xt)
      uint32_t* ar = ln.take();
      rc = run_conv(h, ln, L2, Tb, B, L, R, false, false, src, nullptr, 0, 1.f, lens, at, ar);
      asrc = ar;
    } else {
      rc = run_conv(h, ln, L2, Tb, B, L, nullptr, false, false, src, out, mode, (float)c.n_res,
                    lens, at, aout);
    }
    if (rc) return rc;
  }
  return HFG_OK;
}

// Scratch of the concurrent-ResBlock schedule: per ResBlock its R / Tb and its output.
struct RbConc {
  float* R[HFG_MAX_RES];
  float* Tb[HFG_MAX_RES];
  float* O[HFG_MAX_RES];
};

// Aux streams of one batch part (created on first use; hipStreamNonBlocking)
int rb_streams(hfg_handle* h, int part) {
  for (int j = 0; j < h->cfg.n_res - 1; ++j)
    if (!h->rb_aux[part][j]) {
      hipError_t e = hipStreamCreateWithFlags(&h->rb_aux[part][j], hipStreamNonBlocking);
      if (e == hipSuccess) e = hipEventCreateWithFlags(&h->rb_join[part][j], hipEventDisableTiming);
      if (e != hipSuccess) return hip_fail(e, "create ResBlock stream");
    }
  if (!h->rb_fork[part]) {
    hipError_t e = hipEventCreateWithFlags(&h->rb_fork[part], hipEventDisableTiming);
    if (e != hipSuccess) return hip_fail(e, "create ResBlock fork event");
  }
  return HFG_OK;
}

// MRF of stage st (models/hifigan.py:116-131) on X [B][C][L]: out = mean_j ResBlock_j(X)
// (ResBlock.forward :72-86), or out = ResBlock_only_j(X) alone when only_j >= 0.  R and Tb
// are B*C*L-float scratch buffers of the layer-per-launch ResBlocks; out must not alias X.
// With conc set, the ResBlocks run concurrently (ResBlock j > 0 on aux stream j-1 of this
// batch part), each into its own output, and one combine launch forms the mean in the
// sequential schedule's order — bitwise the same result, for grids that leave CUs idle.
// ax: f16x3 scale slot of X; aout: slot of out (the MRF mean, or ResBlock only_j's output)
int run_mrf(hfg_handle* h, Launcher& ln, const Stage& st, const float* X, int64_t B, int64_t L,
            float* R, float* Tb, float* out, const int32_t* lens, int only_j,
            const uint32_t* ax, uint32_t* aout, const RbConc* conc = nullptr,
            const PostFuse* post = nullptr) {
  const hfg_config& c = h->cfg;
  if (st.thin) return run_thin(h, ln, st, X, B, L, out, lens, only_j, aout);
  int rc;
  if (conc && only_j < 0 && c.n_res > 1) {
    if ((rc = rb_streams(h, ln.part))) return rc;
    hipError_t e = hipEventRecord(h->rb_fork[ln.part], ln.stream);
    for (int j = 1; j < c.n_res && e == hipSuccess; ++j)
      e = hipStreamWaitEvent(h->rb_aux[ln.part][j - 1], h->rb_fork[ln.part], 0);
    if (e != hipSuccess) return hip_fail(e, "ResBlock fork");
    // the ResBlock with the most work (largest kernel-size sum over its dilations) stays on
    // the caller's stream: the aux streams start only after the fork event's cross-queue
    // signal (~10-20 us after the producing launch ends) and the join waits on theirs, so
    // the chain that finishes last should be the one that pays neither (round 6, C1 traces)
    int j_main = 0;
    for (int j = 1; j < c.n_res; ++j)
      if (c.res_kernels[j] * c.n_dil[j] > c.res_kernels[j_main] * c.n_dil[j_main]) j_main = j;
    int idx = 0;
    for (int j = 0, aux = 0; j < c.n_res; ++j) {
      Launcher lj{h, j == j_main ? ln.stream : h->rb_aux[ln.part][aux++], ln.part, ln.seq,
                  c.n_res, ln.sl};
      rc = run_one_rb(h, lj, st, j, idx, X, B, L, conc->R[j], conc->Tb[j], conc->O[j], 0, lens,
                      ax, nullptr);
      if (rc) return rc;
      ln.seq = lj.seq;
      idx += c.n_dil[j];
    }
    for (int j = 1; j < c.n_res && e == hipSuccess; ++j) {
      e = hipEventRecord(h->rb_join[ln.part][j - 1], h->rb_aux[ln.part][j - 1]);
      if (e == hipSuccess) e = hipStreamWaitEvent(ln.stream, h->rb_join[ln.part][j - 1], 0);
    }
    if (e != hipSuccess) return hip_fail(e, "ResBlock join");
    hfg::MrfCombineArgs a{};
    for (int j = 0; j < c.n_res; ++j) a.o[j] = conc->O[j];
    a.n = c.n_res;
    a.C = st.C;
    a.L = (int)L;
    a.len = lens;
    a.y = out;
    a.div = (float)c.n_res;
    a.amax_out = aout;
    ln.begin(0.0, 4.0 * B * L * st.C * (c.n_res + 1));
    e = hfg::launch_mrf_combine(a, (int)B, ln.stream);
    ln.end("mrf_combine");
    if (e != hipSuccess) return hip_fail(e, "launch mrf_combine");
    return HFG_OK;
  }
  int idx = 0;
  for (int j = 0; j < c.n_res; ++j) {
    if (only_j >= 0 && j != only_j) {
      idx += c.n_dil[j];
      continue;
    }
    const int mode = only_j >= 0 ? 0 : ((j > 0 ? 1 : 0) | (j == c.n_res - 1 ? 2 : 0));
    // the write that completes out: the last ResBlock's (the divide), or only_j's
    rc = run_one_rb(h, ln, st, j, idx, X, B, L, R, Tb, out, mode, lens, ax,
                    (only_j >= 0 || (mode & 2)) ? aout : nullptr,
                    only_j < 0 && j == c.n_res - 1 ? post : nullptr);
    if (rc) return rc;
    idx += c.n_dil[j];
  }
  return HFG_OK;
}

// conv_post fused into the last MRF's last ResBlock launch (resblock_bf16x3 conv_post_tail)
// where the plan allows it (RbFused::post): what depends on the call is L % 4 == 0, the
// one-launch-per-ResBlock schedule, and no inspection taps (they read the stage output, which
// that launch does not store)
bool post_fusable(const Stage& st, int64_t L, bool conc_st, float* const* taps) {
  return st.rbs.back().post && !taps && !conc_st && L % 4 == 0;
}

// taps (inspection, hfg_forward_taps): taps[0] <- conv_pre output, taps[1 + 2i] <- ups[i]
// output, taps[2 + 2i] <- mrfs[i] output (models/hifigan.py:238-251); NULL entries skipped.
int forward_impl(hfg_handle* h, const float* mel, int64_t B, int64_t T, const hfg_forward_opts* o,
                 float* wav, int64_t out_len, void* ws, size_t ws_len, hipStream_t stream,
                 int part = 0, float* const* taps = nullptr, bool conc_ok = false) {
  if (!mel || !wav) return fail(HFG_EINVAL, "mel / wav pointer is NULL");
  const bool btc = o && o->mel_layout == HFG_MEL_BTC;
  if (o && o->mel_layout != HFG_MEL_BCT && o->mel_layout != HFG_MEL_BTC)
    return fail(HFG_EINVAL, "unknown mel_layout %d", o->mel_layout);
  const int32_t* user_lens = o ? o->lengths : nullptr;
  if (B <= 0 || T <= 0) return fail(HFG_EINVAL, "B and T must be > 0 (got %lld, %lld)",
                                    (long long)B, (long long)T);
  const Shapes sh = shapes_for(h, B, T);
  for (auto l : sh.L)
    if (l <= 0) return fail(HFG_EINVAL, "T=%lld gives an empty stage", (long long)T);
  if (sh.L.back() != out_len)
    return fail(HFG_EINVAL, "out_len %lld != expected %lld", (long long)out_len,
                (long long)sh.L.back());
  // the kernels address one utterance's activations with 32-bit byte offsets from a
  // per-item base, through buffer descriptors of num_records 0xFFFFFFFF.  The hardware
  // drops a dword whose END passes num_records, so a 4 GiB item would lose its last
  // float: an item holds fewer than 2^30 fp32 elements (V1: T <= 131071 frames)
  if (sh.item_elems >= ((int64_t)1 << 30))
    return fail(HFG_EINVAL, "per-item activation of %lld elements reaches 2^30 (T too long)",
                (long long)sh.item_elems);
  if (ws_len < ws_part_bytes(h, B, T, conc_ok)) return fail(HFG_EINVAL, "workspace too small");
  const int nb = n_bufs(h, B, T, conc_ok);
  float* buf[4 + 3 * HFG_MAX_RES];
  for (int i = 0; i < nb; ++i) buf[i] = reinterpret_cast<float*>(ws) + (size_t)i * sh.buf_elems;
  RbConc conc{};
  for (int j = 0; nb > 4 && j < h->cfg.n_res; ++j) {
    conc.R[j] = buf[4 + 3 * j];
    conc.Tb[j] = buf[5 + 3 * j];
    conc.O[j] = buf[6 + 3 * j];
  }
  float* X = buf[0];    // upsampled stage input
  float* R = buf[1];    // running ResBlock state (also conv_pre output)
  float* Tb = buf[2];   // conv1 output
  float* MRF = buf[3];  // MRF accumulator
  // after the activation buffers: the length table, then the scale slots (ws_part_bytes)
  int32_t* table = reinterpret_cast<int32_t*>(reinterpret_cast<float*>(ws) + (size_t)nb * sh.buf_elems);
  Slots sl;
  Launcher ln{h, stream, part};
  ln.sl = &sl;
  const hfg_config& c = h->cfg;
  int rc = sl.begin(h, reinterpret_cast<char*>(table) + lens_table_bytes(h, B), B, stream);
  if (rc) return rc;
  // ragged batch: per-stage valid lengths, computed on the device from lengths[B]
  const int32_t* lt = nullptr;  // lt + s*B = lengths after s upsample stages
  if (user_lens) {
    hfg::StageLenParams sp{};
    sp.n_up = c.n_up;
    sp.T = (int)T;
    for (int i = 0; i < c.n_up; ++i) {
      sp.up_rates[i] = c.up_rates[i];
      sp.up_kernels[i] = c.up_kernels[i];
    }
    hipError_t e = hfg::launch_stage_lengths(user_lens, (int)B, sp, table, stream);
    if (e != hipSuccess) return fail(HFG_EIO, "launch stage_lengths: %s", hipGetErrorString(e));
    lt = table;
  }
  auto lens_at = [&](int s) { return lt ? lt + (size_t)s * B : nullptr; };
  auto tap = [&](int k, const float* src, int64_t n) -> int {
    if (!taps || !taps[k]) return HFG_OK;
    hipError_t e = hipMemcpyAsync(taps[k], src, sizeof(float) * (size_t)n,
                                  hipMemcpyDeviceToDevice, stream);
    return e == hipSuccess ? HFG_OK : hip_fail(e, "hipMemcpyAsync(tap)");
  };
  // f16x3: the mel's per-item max |value| (no kernel produced it)
  uint32_t* a_mel = ln.take();
  if (a_mel) {
    ln.begin(0.0, 4.0 * B * c.n_mels * T);
    hipError_t e = hfg::launch_absmax(mel, (int64_t)c.n_mels * T, btc ? 1 : T, btc ? c.n_mels : 1,
                                      c.n_mels, (int)T, lens_at(0), (int)B, a_mel, stream);
    ln.end("absmax");
    if (e != hipSuccess) return fail(HFG_EIO, "launch absmax: %s", hipGetErrorString(e));
  }
  // conv_pre  (models/hifigan.py:238)
  uint32_t* a_cur = ln.take();
  rc = run_conv(h, ln, h->layers[h->conv_pre], mel, B, T, R, false, false, nullptr, nullptr, 0,
                1.f, lens_at(0), a_mel, a_cur, btc);
  if (rc) return rc;
  if ((rc = tap(0, R, B * c.c0 * T))) return rc;
  const Layer& Lp = h->layers[h->conv_post];
  const float* cur = R;
  for (int i = 0; i < c.n_up; ++i) {
    const Stage& st = h->stages[i];
    const int64_t Lin = sh.L[i], L = sh.L[i + 1];
    // lrelu -> ups[i]  (models/hifigan.py:244-245)
    uint32_t* a_x = ln.take();
    rc = run_ups(h, ln, h->layers[st.conv_ups], cur, B, Lin, L, X, lens_at(i), lens_at(i + 1),
                 a_cur, a_x);
    if (rc) return rc;
    if ((rc = tap(1 + 2 * i, X, B * st.C * L))) return rc;
    // MRF (models/hifigan.py:116-131) of ResBlocks (:72-86)
    a_cur = ln.take();
    const bool conc_st = nb > 4 && stage_conc(h, st, B, L);
    if (i == c.n_up - 1 && post_fusable(st, L, conc_st, taps)) {
      // the last ResBlock's launch also runs lrelu -> conv_post -> tanh (models/hifigan.py:
      // 254-256); windows past an item's length write nothing: zero the wav first
      if (user_lens) {
        hipError_t e = hipMemsetAsync(wav, 0, sizeof(float) * (size_t)(B * L), stream);
        if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync(wav)");
      }
      const PostFuse pf{h->packed_dev + Lp.pk[0].w_off, h->packed_dev + Lp.pk[0].b_off, wav,
                        post_slope_of(h)};
      rc = run_mrf(h, ln, st, X, B, L, R, Tb, MRF, lens_at(i + 1), -1, a_x, a_cur, nullptr, &pf);
      return rc ? rc : sl.end();
    }
    rc = run_mrf(h, ln, st, X, B, L, R, Tb, MRF, lens_at(i + 1), -1, a_x, a_cur,
                 conc_st ? &conc : nullptr);
    if (rc) return rc;
    if ((rc = tap(2 + 2 * i, MRF, B * st.C * L))) return rc;
    cur = MRF;
  }
  if ((rc = sl.end())) return rc;
  // lrelu -> conv_post -> tanh  (models/hifigan.py:254-256)
  const int64_t L = sh.L.back();
  const char* name = nullptr;
  ln.begin(2.0 * Lp.C_in * 7 * (double)L * B, 4.0 * B * L * (Lp.C_in + 1));
  hipError_t e = hfg::launch_conv_post(cur, (int64_t)Lp.C_in * L, Lp.C_in, (int)L,
                                       h->packed_dev + Lp.pk[0].w_off,
                                       h->packed_dev + Lp.pk[0].b_off, wav, lens_at(c.n_up),
                                       post_slope_of(h), (int)B, stream, &name);
  ln.end(name);
  if (e != hipSuccess) return fail(HFG_EIO, "launch conv_post: %s", hipGetErrorString(e));
  return HFG_OK;
}

}  // namespace

// The forward of a batch: utterances are independent, so a batch of B >= 2 runs as two
// halves on the caller's stream and an internal one (fork / join by events), each half
// with its own workspace slice.  Each wav is bitwise the same as in a one-stream run.
int forward_split(hfg_handle* h, const float* mel, int64_t B, int64_t T,
                  const hfg_forward_opts* o, float* wav, int64_t out_len, void* ws, size_t ws_len,
                  hipStream_t stream) {
  ++h->fwd_count;
  h->halves = split_batch(h, B, T) ? 2 : 1;
  if (h->halves == 1)
    return forward_impl(h, mel, B, T, o, wav, out_len, ws, ws_len, stream, 0, nullptr, true);
  if (B <= 0 || T <= 0) return fail(HFG_EINVAL, "B and T must be > 0");
  if (ws_len < ws_bytes_for(h, B, T)) return fail(HFG_EINVAL, "workspace too small");
  if (!h->aux) {
    hipError_t e = hipStreamCreateWithFlags(&h->aux, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->fork_ev, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->join_ev, hipEventDisableTiming);
    if (e != hipSuccess) return hip_fail(e, "create split stream");
  }
  const int64_t B1 = (B + 1) / 2, B2 = B - B1;
  const size_t w1 = ws_part_bytes(h, B1, T);
  hipStream_t s0 = stream, s1 = h->aux;
  hipError_t e = hipEventRecord(h->fork_ev, stream);
  if (e == hipSuccess) e = hipStreamWaitEvent(s1, h->fork_ev, 0);
  if (e != hipSuccess) return hip_fail(e, "fork");
  int rc = forward_impl(h, mel, B1, T, o, wav, out_len, ws, w1, s0, 0);
  if (rc) return rc;
  hfg_forward_opts o2{};
  if (o) {
    o2 = *o;
    if (o->lengths) o2.lengths = o->lengths + B1;
  }
  rc = forward_impl(h, mel + (size_t)B1 * h->cfg.n_mels * T, B2, T, o ? &o2 : nullptr,
                    wav + (size_t)B1 * out_len, out_len, static_cast<char*>(ws) + w1,
                    ws_len - w1, s1, 1);
  e = hipEventRecord(h->join_ev, s1);
  if (e == hipSuccess) e = hipStreamWaitEvent(stream, h->join_ev, 0);
  if (e != hipSuccess) return hip_fail(e, "join");
  return rc;
}

int forward_taps(hfg_handle* h, const float* mel, int64_t B, int64_t T, float* wav,
                 int64_t out_len, void* ws, size_t ws_len, float* const* taps, hipStream_t stream) {
  ++h->fwd_count;
  h->halves = 1;
  return forward_impl(h, mel, B, T, nullptr, wav, out_len, ws, ws_len, stream, 0, taps,
                      !split_batch(h, B, T));
}

// ---- one MRF / one ResBlock (MRF-only handles, hfg_mrf_create) ---------------
int mrf_run(hfg_handle* h, int only_j, const float* x, int64_t B, int64_t L, float* y, void* ws,
            size_t ws_bytes, hipStream_t st) {
  ++h->fwd_count;
  h->halves = 1;
  const int C = h->stages[0].C;
  const size_t one = (mrf_ws_bytes(h, B, L) - slots_bytes(h, B)) / 2;
  float* R = static_cast<float*>(ws);
  float* Tb = R + one / sizeof(float);
  Slots sl;
  Launcher ln{h, st, 0};
  ln.sl = &sl;
  int rc = sl.begin(h, static_cast<char*>(ws) + 2 * one, B, st);
  if (rc) return rc;
  // f16x3: the caller's x, its per-item max |value| by an absmax pass
  uint32_t* ax = ln.take();
  if (ax) {
    hipError_t e = hfg::launch_absmax(x, (int64_t)C * L, L, 1, C, (int)L, nullptr, (int)B, ax, st);
    if (e != hipSuccess) return fail(HFG_EIO, "launch absmax: %s", hipGetErrorString(e));
  }
  rc = run_mrf(h, ln, h->stages[0], x, B, L, R, Tb, y, nullptr, only_j, ax, nullptr);
  return rc ? rc : sl.end();
}

}  // namespace hfg_host
