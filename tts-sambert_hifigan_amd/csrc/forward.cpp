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

// An activation tensor and the f16x3 scale slot its producer commits (null in the unscaled
// modes, and for a tensor no launch reads a scale of); Src: the same for a tensor only read
// (a caller's input: its slot is written by an absmax pass).
struct Src {
  const float* p = nullptr;
  uint32_t* amax = nullptr;
};
struct Act {
  float* p = nullptr;
  uint32_t* amax = nullptr;
  operator Src() const { return {p, amax}; }
};

// f16x3 activation scales of one forward part (bf16x3_common.h): slot rows handed out in
// launch order; base null in the unscaled modes (every take() is then null)
struct Slots {
  uint32_t* base = nullptr;
  int n = 0, next = 0;
  int64_t B = 0;
  bool overflow = false;
  // the part's slot region (absent unless f16x3), zeroed on the stream
  int begin(const hfg_handle* h, uint32_t* at, const WsPart& part, hipStream_t stream) {
    if (!(base = at)) return HFG_OK;
    n = n_slots(h);
    B = part.B;
    hipError_t e = hipMemsetAsync(base, 0, part.slots.bytes, stream);
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
  void* ws;  // the caller's workspace
  hipStream_t stream;
  int part = 0;
  int seq = 0;
  int conc = 1;  // launches of this schedule running side by side (concurrent ResBlocks)
  Slots* sl = nullptr;
  ProfRec* rec = nullptr;
  // The one "base + offset" into the workspace: every pointer of a forward is a region of
  // its layout (handle.h, WsLayout); null for an absent region.
  template <class T>
  T* at(const WsRegion& r) const {
    return r.bytes ? reinterpret_cast<T*>(static_cast<char*>(ws) + r.off) : nullptr;
  }
  // the tensor the next producing launch writes, with the next scale slot
  Act act(float* p) { return {p, sl ? sl->take() : nullptr}; }
  Src act(const float* p) { return {p, sl ? sl->take() : nullptr}; }
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

// What is constant for one stage of one part: the batch, the stage's length and the row of
// the part's length table (null: every item L long).
struct Dims {
  int64_t B, L;
  const int32_t* lens;
};

// What a Conv1d and a polyphase ConvTranspose1d launch share: x [B][C_in][in.L] ->
// y [B][C_out][out.L] as a GEMM of L.M rows x L.KT taps, each side with its scale slot.
ConvParams layer_params(const hfg_handle* h, const Layer& L, const Dims& in, Src x,
                        const Dims& out, Act y) {
  ConvParams p{};
  p.x = x.p;
  p.x_bs = (int64_t)L.C_in * in.L;
  p.x_cs = in.L;
  p.x_ts = 1;
  p.C_in = L.C_in;
  p.L_in = (int)in.L;
  p.len_in = in.lens;
  p.len_out = out.lens;
  p.y = y.p;
  p.y_bs = (int64_t)L.C_out * out.L;
  p.M = L.M;
  p.dil = L.dil;
  p.kt = L.KT;
  p.amax_in = x.amax;
  p.amax_out = y.amax;
  p.ew = L.ew;
  p.dbg = h->dbg_flags;
  return p;
}

// The launch of a layer whose p.N output columns are set: the packing (a split-precision
// layer whose own tile would leave most CUs idle, fewer than kSmallGridBlocks blocks over
// the `conc` launches that share the chip, runs the small tile on its own packing: bitwise
// the same result, kernels.h tile 4), the profile record, the kernel of the layer's precision.
int launch_layer(Launcher& ln, const Layer& L, ConvParams& p, bool ups, int64_t B, double flop,
                 double bytes) {
  hfg_handle* h = ln.h;
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
  p.w = h->packed_dev + pk->w.off;
  p.bias = h->packed_dev + pk->b.off;
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

struct PostFuse {
  const float* w;  // conv_post weight [C][7], bias [1] (packed fp32)
  const float* b;
  float* wav;      // [B][L]
  float slope;     // of the leaky_relu in front of conv_post (post_slope_of)
};

// Where a ResBlock's result goes in the MRF: y combined by the epilogue mode (bit0 add, bit1
// divide by div), amax the slot of y where this write completes it, post the conv_post +
// tanh fused into a whole-ResBlock launch that is the network's last MRF write.
struct MrfOut {
  float* y = nullptr;
  int mode = 0;
  float div = 1.f;
  uint32_t* amax = nullptr;
  const PostFuse* post = nullptr;
};

// What a conv launch does around its GEMM, named where it is asked for.
struct ConvOpts {
  bool act_in = false, act_out = false, x_btc = false;
  const float* res = nullptr;
  ConvOpts& lrelu_in() { return act_in = true, *this; }
  ConvOpts& lrelu_out() { return act_out = true, *this; }
  ConvOpts& residual(const float* r) { return res = r, *this; }
  // x is [B][T][C] (acoustic-model layout) instead of [B][C][T]
  ConvOpts& btc_input(bool on) { return x_btc = on, *this; }
};

// One conv-layer launch (regular Conv1d): y = conv(x), or with mrf the ResBlock's last conv,
// whose result goes to the MRF epilogue instead of y.
int run_conv(Launcher& ln, const Layer& L, const Dims& d, Src x, Act y, const ConvOpts& o,
             const MrfOut* mrf = nullptr) {
  if (mrf) y = Act{nullptr, mrf->amax};
  ConvParams p = layer_params(ln.h, L, d, x, d, y);
  if (o.x_btc) {
    p.x_cs = 1;
    p.x_ts = L.C_in;
  }
  const int64_t B = d.B, Lt = d.L;
  p.N = (int)Lt;
  p.off = -L.pad;
  p.act_in = o.act_in;
  p.act_out = o.act_out;
  p.res = o.res;
  p.mrf = mrf ? mrf->y : nullptr;
  p.mrf_mode = mrf ? mrf->mode : 0;
  p.mrf_div = mrf ? mrf->div : 1.f;
  p.epi_lds = 1;
  const double flop = 2.0 * L.C_out * L.C_in * L.k * (double)Lt * B;
  double bytes = 4.0 * B * Lt * (L.C_in + L.C_out) + 4.0 * L.C_out * L.C_in * L.k;
  if (o.res) bytes += 4.0 * B * Lt * L.C_out;
  if (mrf && (mrf->mode & 1)) bytes += 4.0 * B * Lt * L.C_out;
  return launch_layer(ln, L, p, false, B, flop, bytes);
}

// slope of the leaky_relu in front of conv_post: the reference's 0.1 (models/hifigan.py:254)
// unless the config names another (the public release's F.leaky_relu(x) default, 0.01)
inline float post_slope_of(const hfg_handle* h) {
  return h->cfg.post_slope ? h->cfg.post_slope : hfg::kLReluSlope;
}

// One whole ResBlock (all dilations) + its MRF contribution in one launch.
// A split ResBlock (rb.split) runs as two launches through `scratch` (B*C*L floats): convs
// [0, split) write x after their dilation pairs (MRF-epilogue mode 0: a plain store), convs
// [split, n) read it back and do the MRF epilogue.  fp32 round trip: bitwise the same x.
// out.post: conv_post + tanh fused into the last launch (C = 32, the network's last MRF write).
int run_resblock(Launcher& ln, const RbFused& rb, const Dims& d, const float* x, float* scratch,
                 const MrfOut& out) {
  hfg_handle* h = ln.h;
  const int64_t B = d.B, Lt = d.L;
  const PostFuse* post = out.post;
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
    p.len = d.lens;
    p.w = reinterpret_cast<const __bf16*>(h->packed_dev + rb.w.off);
    p.w_bytes = (int)(rb.w.len * sizeof(float));
    p.bias = h->packed_dev + rb.b.off + hfg::pack_bias_convs(c0, C);
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
    p.mrf = last ? out.y : scratch;
    p.mrf_mode = last ? out.mode : 0;
    p.mrf_div = out.div;
    p.mrf_rcp = hfg::fast_div_ok(out.div) ? 1.0f / out.div : 0.0f;
    p.amax_out = last ? out.amax : nullptr;
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
        4.0 * B * Lt * C * ((last && (out.mode & 1)) ? 3 : 2) + 4.0 * (double)rb.w.len;
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

// lrelu -> ConvTranspose1d: x [B][C_in][in.L] -> y [B][C_out][out.L]
int run_ups(Launcher& ln, const Layer& L, const Dims& in, Src x, const Dims& out, Act y) {
  hfg_handle* h = ln.h;
  const int64_t B = in.B, Lin = in.L, Lout = out.L;
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
      q.x = x.p;
      q.x_bs = (int64_t)L.C_in * Lin;
      q.C_in = L.C_in;
      q.L = (int)Lin;
      q.T = (int)Lin;
      q.len_in = in.lens;
      q.w = reinterpret_cast<const __bf16*>(h->packed_dev + L.wf.off);
      q.bias = h->packed_dev + L.bf.off;
      q.y = y.p;
      q.y_bs = (int64_t)L.C_out * Lout;
      q.C_out = L.C_out;
      q.L_out = (int)Lout;
      q.u = L.s;
      q.m_tiles = L.m_tiles_f;
      q.n_tiles = n_tiles;
      q.batch = (int)B;
      q.amax_in = x.amax;
      q.amax_out = y.amax;
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
  ConvParams p = layer_params(h, L, in, x, out, y);
  // columns u: t_out + p = s*u + r  for t_out in [0, Lout)
  p.N = (int)((Lout - 1 + L.p) / L.s + 1);
  p.off = -(L.KT - 1);
  p.act_in = 1;  // F.leaky_relu before every upsample, models/hifigan.py:244
  p.ups_s = L.s;
  p.ups_p = L.p;
  p.ups_swz = 1;
  p.L_out = (int)Lout;
  return launch_layer(ln, L, p, true, B, flop, bytes);
}

// A thin stage's whole MRF (or ResBlock only_j alone) in one mrf_thin launch.
int run_thin(Launcher& ln, const Stage& st, const Dims& d, const float* X, Act out, int only_j) {
  hfg_handle* h = ln.h;
  const int64_t B = d.B, Lt = d.L;
  const hfg_config& c = h->cfg;
  const int C = st.C;
  hfg::ThinParams p{};
  p.x = X;
  p.bs = (int64_t)C * Lt;
  p.L = (int)Lt;
  p.len = d.lens;
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
    p.w_off[q] = (int)st.thin_w[e].off;
    flop += 2.0 * C * C * L.k * (double)Lt * B;
    wbytes += 4.0 * C * C * L.k;
  }
  // the kernel indexes biases as [conv][C] from this launch's first conv
  p.bias = h->packed_dev + st.thin_b.off + hfg::pack_bias_convs(cv_base, C);
  p.halo = halo;
  p.W = (st.thin_mfma ? hfg::thin_mfma_window(C) : hfg::thin_window(C)) - 2 * halo;
  p.y = out.p;
  p.div = (float)p.n_res;
  p.amax_out = out.amax;
  if (st.thin_mfma) {
    const int base = st.thin_m_conv[cv_base];
    p.wm = reinterpret_cast<const __bf16*>(h->packed_dev + st.thin_m.off) + base / 2;
    p.wm_bytes = (int)(st.thin_m.len * sizeof(float)) - base;
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
// combined into the MRF as `out` says; b: scratch of the layer-per-launch path (b.Tb: also of
// a split whole-ResBlock launch).
int run_one_rb(Launcher& ln, const Stage& st, int j, const Dims& d, Src X, const WsRbRegions& b,
               const MrfOut& out) {
  hfg_handle* h = ln.h;
  const hfg_config& c = h->cfg;
  float *R = ln.at<float>(b.R), *Tb = ln.at<float>(b.Tb);
  if (st.rbs[j].fused) return run_resblock(ln, st.rbs[j], d, X.p, Tb, out);
  // index of the block's first dilation in st.conv1 / st.conv2
  int idx = 0;
  for (int q = 0; q < j; ++q) idx += c.n_dil[q];
  int rc;
  Src src = X;
  for (int m = 0; m < c.n_dil[j]; ++m, ++idx) {
    const bool last = m == c.n_dil[j] - 1;
    const Layer& L1 = h->layers[st.conv1[idx]];
    if (c.resblock_type == 1) {
      // ResBlock2, one launch per dilation: x = x + conv_m(lrelu(x)).  The conv reads a
      // neighbourhood of x, so it writes the other of R / Tb; the last one carries the MRF epilogue
      const Act dst = last ? Act{} : ln.act((m & 1) ? Tb : R);
      rc = run_conv(ln, L1, d, src, dst, ConvOpts().lrelu_in().residual(src.p),
                    last ? &out : nullptr);
      if (rc) return rc;
      src = dst;
      continue;
    }
    // xt = lrelu(conv1(lrelu(x)))
    const Act xt = ln.act(Tb);
    if ((rc = run_conv(ln, L1, d, src, xt, ConvOpts().lrelu_in().lrelu_out()))) return rc;
    // x = x + conv2(xt); the last one carries the MRF epilogue
    const Act x = last ? Act{} : ln.act(R);
    rc = run_conv(ln, h->layers[st.conv2[idx]], d, xt, x, ConvOpts().residual(src.p),
                  last ? &out : nullptr);
    if (rc) return rc;
    src = x;
  }
  return HFG_OK;
}

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

// The scratch of one MRF: seq for ResBlocks run one after another (or only_j alone), conc
// (null: that schedule is off) one entry per ResBlock run side by side.
struct MrfBufs {
  const WsRbRegions& seq;
  const WsRbRegions* conc = nullptr;
};

// MRF of stage st (models/hifigan.py:116-131) on X [B][C][L]: out = mean_j ResBlock_j(X)
// (ResBlock.forward :72-86), or out = ResBlock_only_j(X) alone when only_j >= 0; out must not
// alias X.  With bufs.conc set, the ResBlocks run concurrently (ResBlock j > 0 on aux stream
// j-1 of this batch part), each into its own output, and one combine launch forms the mean in
// the sequential schedule's order — bitwise the same result, for grids that leave CUs idle.
// post: conv_post + tanh in the last ResBlock's launch (sequential schedule only).
int run_mrf(Launcher& ln, const Stage& st, const Dims& d, Src X, const MrfBufs& bufs, Act out,
            int only_j, const PostFuse* post = nullptr) {
  hfg_handle* h = ln.h;
  const hfg_config& c = h->cfg;
  if (st.thin) return run_thin(ln, st, d, X.p, out, only_j);
  int rc;
  if (bufs.conc && only_j < 0 && c.n_res > 1) {
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
    hfg::MrfCombineArgs a{};
    for (int j = 0, aux = 0; j < c.n_res; ++j) {
      Launcher lj{h, ln.ws, j == j_main ? ln.stream : h->rb_aux[ln.part][aux++], ln.part, ln.seq,
                  c.n_res, ln.sl};
      // mode 0: a plain store of the block's result
      const MrfOut own{ln.at<float>(bufs.conc[j].out), 0, (float)c.n_res};
      if ((rc = run_one_rb(lj, st, j, d, X, bufs.conc[j], own))) return rc;
      ln.seq = lj.seq;
      a.o[j] = own.y;
    }
    for (int j = 1; j < c.n_res && e == hipSuccess; ++j) {
      e = hipEventRecord(h->rb_join[ln.part][j - 1], h->rb_aux[ln.part][j - 1]);
      if (e == hipSuccess) e = hipStreamWaitEvent(ln.stream, h->rb_join[ln.part][j - 1], 0);
    }
    if (e != hipSuccess) return hip_fail(e, "ResBlock join");
    a.n = c.n_res;
    a.C = st.C;
    a.L = (int)d.L;
    a.len = d.lens;
    a.y = out.p;
    a.div = (float)c.n_res;
    a.amax_out = out.amax;
    ln.begin(0.0, 4.0 * d.B * d.L * st.C * (c.n_res + 1));
    e = hfg::launch_mrf_combine(a, (int)d.B, ln.stream);
    ln.end("mrf_combine");
    if (e != hipSuccess) return hip_fail(e, "launch mrf_combine");
    return HFG_OK;
  }
  for (int j = 0; j < c.n_res; ++j) {
    if (only_j >= 0 && j != only_j) continue;
    const bool last = j == c.n_res - 1;
    const int mode = only_j >= 0 ? 0 : ((j > 0 ? 1 : 0) | (last ? 2 : 0));
    // the slot goes with the write that completes out: the last ResBlock's (the divide), or
    // only_j's; conv_post with the last ResBlock's
    const MrfOut to{out.p, mode, (float)c.n_res, only_j >= 0 || last ? out.amax : nullptr,
                    only_j < 0 && last ? post : nullptr};
    if ((rc = run_one_rb(ln, st, j, d, X, bufs.seq, to))) return rc;
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

// What every generator forward checks before it touches the workspace; *sh <- the shapes.
int check_forward(const hfg_handle* h, const FwdIo& io, Shapes* sh) {
  if (!io.mel || !io.wav) return fail(HFG_EINVAL, "mel / wav pointer is NULL");
  const hfg_forward_opts* o = io.opts;
  if (o && o->mel_layout != HFG_MEL_BCT && o->mel_layout != HFG_MEL_BTC)
    return fail(HFG_EINVAL, "unknown mel_layout %d", o->mel_layout);
  if (io.B <= 0 || io.T <= 0) return fail(HFG_EINVAL, "B and T must be > 0 (got %lld, %lld)",
                                          (long long)io.B, (long long)io.T);
  // the batch is a grid's y or z dimension
  if (io.B > kMaxBatch) return fail(HFG_EINVAL, "B must be in [1, 65535] (got %lld)",
                                    (long long)io.B);
  *sh = shapes_for(h, io.T);
  for (auto l : sh->L)
    if (l <= 0) return fail(HFG_EINVAL, "T=%lld gives an empty stage", (long long)io.T);
  if (sh->L.back() != io.out_len)
    return fail(HFG_EINVAL, "out_len %lld != expected %lld", (long long)io.out_len,
                (long long)sh->L.back());
  // the kernels address one utterance's activations with 32-bit byte offsets from a
  // per-item base, through buffer descriptors of num_records 0xFFFFFFFF.  The hardware
  // drops a dword whose END passes num_records, so a 4 GiB item would lose its last
  // float: an item holds fewer than 2^30 fp32 elements (V1: T <= 131071 frames)
  if (sh->item_elems >= ((int64_t)1 << 30))
    return fail(HFG_EINVAL, "per-item activation of %lld elements reaches 2^30 (T too long)",
                (long long)sh->item_elems);
  return HFG_OK;
}

// One part of a checked forward (items [part.b0, part.b0 + part.B) of io) on `stream`, every
// buffer a region of `part`; L: the stage lengths (Shapes::L).
// taps (inspection, hfg_forward_taps): taps[0] <- conv_pre output, taps[1 + 2i] <- ups[i]
// output, taps[2 + 2i] <- mrfs[i] output (models/hifigan.py:238-251); NULL entries skipped.
int forward_part(Launcher& ln, const FwdIo& io, const std::vector<int64_t>& L, const WsPart& part) {
  hfg_handle* h = ln.h;
  hipStream_t stream = ln.stream;
  const hfg_config& c = h->cfg;
  const int64_t B = part.B, T = io.T;
  const bool btc = io.opts && io.opts->mel_layout == HFG_MEL_BTC;
  const int32_t* user_lens = io.opts && io.opts->lengths ? io.opts->lengths + part.b0 : nullptr;
  const float* mel = io.mel + (size_t)part.b0 * c.n_mels * T;
  float* wav = io.wav + (size_t)part.b0 * io.out_len;
  float* const* taps = io.taps;
  MrfBufs bufs{part.rb};  // (part.rb.out: the MRF accumulator)
  int32_t* table = ln.at<int32_t>(part.table);
  Slots sl;
  ln.sl = &sl;
  int rc = sl.begin(h, ln.at<uint32_t>(part.slots), part, stream);
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
  // stage s of this part: L[s] long, its row of the length table
  auto dims = [&](int s) { return Dims{B, L[s], lt ? lt + (size_t)s * B : nullptr}; };
  auto tap = [&](int k, const float* src, int64_t n) -> int {
    if (!taps || !taps[k]) return HFG_OK;
    hipError_t e = hipMemcpyAsync(taps[k], src, sizeof(float) * (size_t)n,
                                  hipMemcpyDeviceToDevice, stream);
    return e == hipSuccess ? HFG_OK : hip_fail(e, "hipMemcpyAsync(tap)");
  };
  // f16x3: the mel's per-item max |value| (no kernel produced it)
  const Src m = ln.act(mel);
  if (m.amax) {
    ln.begin(0.0, 4.0 * B * c.n_mels * T);
    hipError_t e = hfg::launch_absmax(mel, (int64_t)c.n_mels * T, btc ? 1 : T, btc ? c.n_mels : 1,
                                      c.n_mels, (int)T, dims(0).lens, (int)B, m.amax, stream);
    ln.end("absmax");
    if (e != hipSuccess) return fail(HFG_EIO, "launch absmax: %s", hipGetErrorString(e));
  }
  // conv_pre  (models/hifigan.py:238), into R
  Act cur = ln.act(ln.at<float>(part.rb.R));
  rc = run_conv(ln, h->layers[h->conv_pre], dims(0), m, cur, ConvOpts().btc_input(btc));
  if (rc) return rc;
  if ((rc = tap(0, cur.p, B * c.c0 * T))) return rc;
  const Layer& Lp = h->layers[h->conv_post];
  for (int i = 0; i < c.n_up; ++i) {
    const Stage& st = h->stages[i];
    const Dims d = dims(i + 1);
    // lrelu -> ups[i]  (models/hifigan.py:244-245)
    const Act x = ln.act(ln.at<float>(part.X));
    if ((rc = run_ups(ln, h->layers[st.conv_ups], dims(i), cur, d, x))) return rc;
    if ((rc = tap(1 + 2 * i, x.p, B * st.C * d.L))) return rc;
    // MRF (models/hifigan.py:116-131) of ResBlocks (:72-86)
    cur = ln.act(ln.at<float>(part.rb.out));
    const bool conc_st = part.conc && stage_conc(h, st, B, d.L);
    bufs.conc = conc_st ? part.rb_conc : nullptr;
    if (i == c.n_up - 1 && post_fusable(st, d.L, conc_st, taps)) {
      // the last ResBlock's launch also runs lrelu -> conv_post -> tanh (models/hifigan.py:
      // 254-256); windows past an item's length write nothing: zero the wav first
      if (user_lens) {
        hipError_t e = hipMemsetAsync(wav, 0, sizeof(float) * (size_t)(B * d.L), stream);
        if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync(wav)");
      }
      const PostFuse pf{h->packed_dev + Lp.pk[0].w.off, h->packed_dev + Lp.pk[0].b.off, wav,
                        post_slope_of(h)};
      rc = run_mrf(ln, st, d, x, bufs, cur, -1, &pf);
      return rc ? rc : sl.end();
    }
    if ((rc = run_mrf(ln, st, d, x, bufs, cur, -1))) return rc;
    if ((rc = tap(2 + 2 * i, cur.p, B * st.C * d.L))) return rc;
  }
  if ((rc = sl.end())) return rc;
  // lrelu -> conv_post -> tanh  (models/hifigan.py:254-256)
  const Dims d = dims(c.n_up);
  const char* name = nullptr;
  ln.begin(2.0 * Lp.C_in * 7 * (double)d.L * B, 4.0 * B * d.L * (Lp.C_in + 1));
  hipError_t e = hfg::launch_conv_post(cur.p, (int64_t)Lp.C_in * d.L, Lp.C_in, (int)d.L,
                                       h->packed_dev + Lp.pk[0].w.off,
                                       h->packed_dev + Lp.pk[0].b.off, wav, d.lens,
                                       post_slope_of(h), (int)B, stream, &name);
  ln.end(name);
  if (e != hipSuccess) return fail(HFG_EIO, "launch conv_post: %s", hipGetErrorString(e));
  return HFG_OK;
}

}  // namespace

// A checked forward over its layout: one part on the caller's stream, or (utterances are
// independent) two batch halves on the caller's stream and an internal one, fork / join by
// events, each half with its own part of the workspace.  Each wav is bitwise the same as in a
// one-stream run.
int forward_run(hfg_handle* h, const FwdIo& io, void* ws, size_t ws_len, hipStream_t stream,
                bool taps) {
  ++h->fwd_count;
  Shapes sh;
  int rc = check_forward(h, io, &sh);
  if (rc) return rc;
  const WsLayout lay = ws_layout(h, io.B, io.T, taps);
  if (ws_len < lay.total) return fail(HFG_EINVAL, "workspace too small");
  h->halves = lay.n_parts;
  Launcher l0{h, ws, stream, 0};
  if (lay.n_parts == 1) return forward_part(l0, io, sh.L, lay.part[0]);
  if (!h->aux) {
    hipError_t e = hipStreamCreateWithFlags(&h->aux, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->fork_ev, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->join_ev, hipEventDisableTiming);
    if (e != hipSuccess) return hip_fail(e, "create split stream");
  }
  hipError_t e = hipEventRecord(h->fork_ev, stream);
  if (e == hipSuccess) e = hipStreamWaitEvent(h->aux, h->fork_ev, 0);
  if (e != hipSuccess) return hip_fail(e, "fork");
  if ((rc = forward_part(l0, io, sh.L, lay.part[0]))) return rc;
  Launcher l1{h, ws, h->aux, 1};
  rc = forward_part(l1, io, sh.L, lay.part[1]);
  e = hipEventRecord(h->join_ev, h->aux);
  if (e == hipSuccess) e = hipStreamWaitEvent(stream, h->join_ev, 0);
  if (e != hipSuccess) return hip_fail(e, "join");
  return rc;
}

// ---- one MRF / one ResBlock (MRF-only handles, hfg_mrf_create) ---------------
int mrf_run(hfg_handle* h, int only_j, const float* x_in, int64_t L, float* y, const WsPart& part,
            void* ws, hipStream_t st) {
  ++h->fwd_count;
  h->halves = 1;
  const int C = h->stages[0].C;
  const int64_t B = part.B;
  Slots sl;
  Launcher ln{h, ws, st, 0};
  ln.sl = &sl;
  int rc = sl.begin(h, ln.at<uint32_t>(part.slots), part, st);
  if (rc) return rc;
  // f16x3: the caller's x, its per-item max |value| by an absmax pass
  const Src x = ln.act(x_in);
  if (x.amax) {
    hipError_t e =
        hfg::launch_absmax(x.p, (int64_t)C * L, L, 1, C, (int)L, nullptr, (int)B, x.amax, st);
    if (e != hipSuccess) return fail(HFG_EIO, "launch absmax: %s", hipGetErrorString(e));
  }
  // (no consumer of y's scale)
  rc = run_mrf(ln, h->stages[0], Dims{B, L, nullptr}, x, MrfBufs{part.rb}, Act{y, nullptr},
               only_j);
  return rc ? rc : sl.end();
}

}  // namespace hfg_host
