// inspect_capi.cpp — the C ABI of include/hifigan_hip_inspect.h (hfg_probe_mfma_rate apart:
// probe.hip): the packed-image copy-outs, the plan and workspace descriptions, the LDS sizes,
// the tap forward and the schedule-knob store.  What the host suite and the measurement tools
// look at; nothing here is on a forward's path but sched_apply, read when a handle is created.
#include <algorithm>
#include <cstring>

#include "handle.h"
#include "json_writer.h"
#include "mel_kernels.h"

using namespace hfg_host;
using hfg::kTiles;

namespace {
std::mutex g_sched_mu;
std::map<std::string, int> g_sched;

const SchedKnob* sched_knob(const char* name) {
  if (!name) return nullptr;
  for (const SchedKnob& k : kSchedKnobs)
    if (!strcmp(k.name, name)) return &k;
  return nullptr;
}

int commit_if_dirty(hfg_handle* h) { return h->dirty ? do_commit(h) : HFG_OK; }

// How a copy-out ends: pending weights committed, then the weights w and the biases b of the
// packed host image into out[cap]
int copy_packed(hfg_handle* h, float* out, size_t cap, const PackRegion& w, const PackRegion& b) {
  int rc = commit_if_dirty(h);
  if (rc) return rc;
  if (cap < w.len + b.len) return fail(HFG_EINVAL, "output buffer too small");
  memcpy(out, h->packed_host.data() + w.off, sizeof(float) * w.len);
  memcpy(out + w.len, h->packed_host.data() + b.off, sizeof(float) * b.len);
  return HFG_OK;
}

// sha256 of n bytes as 64 hex digits (FIPS 180-4), for hfg_debug_plan
std::string sha256_hex(const unsigned char* d, size_t n) {
  static const uint32_t K[64] = {
      0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5,
      0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174,
      0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da,
      0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967,
      0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
      0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070,
      0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3,
      0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
  uint32_t s[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a,
                   0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
  auto rotr = [](uint32_t x, int r) { return (x >> r) | (x << (32 - r)); };
  // the message, then 0x80, zeros and the 64-bit big-endian bit count, in 64-byte blocks
  const size_t total = (n + 9 + 63) / 64 * 64;
  for (size_t b0 = 0; b0 < total; b0 += 64) {
    uint32_t w[64];
    for (int i = 0; i < 16; ++i) {
      w[i] = 0;
      for (int q = 0; q < 4; ++q) {
        const size_t at = b0 + 4 * i + q;
        const uint32_t byte = at < n    ? d[at]
                              : at == n ? 0x80u
                              : at >= total - 8 ? (uint32_t)(((uint64_t)n * 8) >> (8 * (total - 1 - at))) & 0xffu
                                                : 0u;
        w[i] = (w[i] << 8) | byte;
      }
    }
    for (int i = 16; i < 64; ++i)
      w[i] = w[i - 16] + (rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3)) + w[i - 7] +
             (rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10));
    uint32_t v[8];
    memcpy(v, s, sizeof(v));
    for (int i = 0; i < 64; ++i) {
      const uint32_t t1 = v[7] + (rotr(v[4], 6) ^ rotr(v[4], 11) ^ rotr(v[4], 25)) +
                          ((v[4] & v[5]) ^ (~v[4] & v[6])) + K[i] + w[i];
      const uint32_t t2 = (rotr(v[0], 2) ^ rotr(v[0], 13) ^ rotr(v[0], 22)) +
                          ((v[0] & v[1]) ^ (v[0] & v[2]) ^ (v[1] & v[2]));
      for (int q = 7; q > 0; --q) v[q] = v[q - 1];
      v[4] += t1;
      v[0] = t1 + t2;
    }
    for (int q = 0; q < 8; ++q) s[q] += v[q];
  }
  char hex[65];
  for (int q = 0; q < 8; ++q) snprintf(hex + 8 * q, 9, "%08x", s[q]);
  return hex;
}
}  // namespace

namespace hfg_host {
void sched_apply(const char* knob, int* v) {
  std::lock_guard<std::mutex> lk(g_sched_mu);
  auto it = g_sched.find(knob);
  if (it != g_sched.end()) *v = it->second;
}
void sched_apply(const char* knob, bool* v) {
  int i = *v ? 1 : 0;
  sched_apply(knob, &i);
  *v = i != 0;
}
}  // namespace hfg_host

extern "C" {

int hfg_debug_schedule_set(const char* knob, int value) {
  const SchedKnob* k = sched_knob(knob);
  if (!k) return fail(HFG_EINVAL, "unknown schedule knob '%s'", knob ? knob : "(null)");
  if (value < k->lo || value > k->hi)
    return fail(HFG_EINVAL, "schedule knob %s = %d out of range [%d, %d]%s", k->name, value,
                k->lo, k->hi,
                !strcmp(k->name, "UPS_FRAMES") && value == 0
                    ? " (0, the polyphase-only upsampler schedule, was removed in round 4)"
                    : "");
  std::lock_guard<std::mutex> lk(g_sched_mu);
  g_sched[k->name] = value;
  return HFG_OK;
}

int hfg_debug_schedule_clear(const char* knob) {
  if (knob && !sched_knob(knob)) return fail(HFG_EINVAL, "unknown schedule knob '%s'", knob);
  std::lock_guard<std::mutex> lk(g_sched_mu);
  if (knob)
    g_sched.erase(knob);
  else
    g_sched.clear();
  return HFG_OK;
}

int hfg_debug_schedule_get(const char* knob, int* value) {
  if (!sched_knob(knob) || !value) return fail(HFG_EINVAL, "unknown schedule knob or NULL value");
  std::lock_guard<std::mutex> lk(g_sched_mu);
  auto it = g_sched.find(knob);
  if (it == g_sched.end()) return 0;
  *value = it->second;
  return 1;
}

const char* hfg_debug_schedule_knob(int i) {
  const int n = (int)(sizeof(kSchedKnobs) / sizeof(kSchedKnobs[0]));
  return i >= 0 && i < n ? kSchedKnobs[i].name : nullptr;
}

// Copy the packed host image of layer `name` (module prefix) for host tests.
int hfg_debug_packed_layer(hfg_handle* h, const char* mod, float* out, size_t cap,
                           int64_t* info) {
  if (!h || !mod) return fail(HFG_EINVAL, "NULL argument");
  // "<module>#small": the layer's small-grid-tile packing; "<module>#frames": the output-frame
  // upsampler's (ups_bf16x3) — HFG_EINVAL where the plan has none
  std::string name(mod);
  int which = 0;
  const size_t hash = name.find('#');
  if (hash != std::string::npos) {
    const std::string sel = name.substr(hash + 1);
    which = sel == "small" ? 1 : sel == "frames" ? 2 : -1;
    if (which < 0) return fail(HFG_EINVAL, "unknown packing '%s' (small, frames)", sel.c_str());
    name.resize(hash);
  }
  std::lock_guard<std::recursive_mutex> lk(h->mu);
  for (auto& L : h->layers) {
    if (L.mod != name) continue;
    if (which == 2) {
      if (L.ups_cfg < 0) return fail(HFG_EINVAL, "%s has no output-frame packing", name.c_str());
      if (info) {
        const int64_t v[10] = {L.kind, (int64_t)L.C_out * L.s / 2, 2, L.ups_cfg, L.m_tiles_f,
                               L.C_in / 16, (int64_t)L.wf.len, (int64_t)L.bf.len, 16,
                               hfg::kUpsCfgs[L.ups_cfg].MT()};
        std::copy_n(v, 10, info);
      }
      return out ? copy_packed(h, out, cap, L.wf, L.bf) : HFG_OK;
    }
    const Packing& pk = L.pk[which];
    if (which == 1 && pk.tile < 0)
      return fail(HFG_EINVAL, "%s has no small-tile packing", name.c_str());
    if (info) {
      info[0] = L.kind;
      info[1] = L.M;
      info[2] = L.KT;
      info[3] = pk.tile;
      info[4] = pk.m_tiles;
      info[5] = pk.n_chunks;
      info[6] = (int64_t)pk.w.len;
      info[7] = (int64_t)pk.b.len;
      info[8] = L.CK;
      info[9] = L.kind == L_POST ? 0
                : L.prec == 1    ? hfg::kBf16x3Tiles[pk.tile].MT()
                                 : kTiles[pk.tile].MT();
    }
    return out ? copy_packed(h, out, cap, pk.w, pk.b) : HFG_OK;
  }
  return fail(HFG_EINVAL, "unknown layer '%s'", mod);
}

// The f16x3 packing exponent of layer `mod` (0 in the other modes): set by the commit, so a
// handle with uncommitted weights commits first and returns its error (e.g. weights missing).
int hfg_debug_layer_exponent(hfg_handle* h, const char* mod, int* ew) {
  if (!h || !mod || !ew) return fail(HFG_EINVAL, "NULL argument");
  std::lock_guard<std::recursive_mutex> lk(h->mu);
  for (auto& L : h->layers) {
    if (L.mod != mod) continue;
    int rc = commit_if_dirty(h);
    if (rc) return rc;
    *ew = L.ew;
    return HFG_OK;
  }
  return fail(HFG_EINVAL, "unknown layer '%s'", mod);
}

int hfg_debug_packed_resblock(hfg_handle* h, int stage, int j, float* out, size_t cap,
                              int64_t* info) {
  if (!h || !info) return fail(HFG_EINVAL, "NULL argument");
  std::lock_guard<std::recursive_mutex> lk(h->mu);
  if (stage < 0 || stage >= (int)h->stages.size()) return fail(HFG_EINVAL, "stage out of range");
  const Stage& st = h->stages[stage];
  for (int i = 0; i < 8; ++i) info[i] = 0;
  if (j < 0 || j >= (int)st.rbs.size()) return fail(HFG_EINVAL, "resblock out of range");
  const RbFused& rb = st.rbs[j];
  if (!rb.fused) return HFG_OK;
  info[0] = 1;  // fused (resblock_bf16x3 stream order)
  info[1] = h->layers[rb.convs[0]].C_out;
  info[2] = rb.kt;
  info[3] = (int64_t)rb.convs.size();
  info[4] = rb.halo;
  info[5] = rb.W;
  info[6] = (int64_t)rb.w.len;
  info[7] = (int64_t)rb.b.len;
  return out ? copy_packed(h, out, cap, rb.w, rb.b) : HFG_OK;
}

int hfg_debug_thin_window(int C, int mfma) {
  return mfma ? hfg::thin_mfma_window(C) : hfg::thin_window(C);
}

// What each launcher passes as dynamic LDS (the total of its kernel's layout, lds_layout.h),
// by the same functions the launchers call.
int64_t hfg_debug_lds_bytes(const char* family, const int* a, int n) {
  using namespace hfg;
  if (!family || !a) return -1;
  const std::string f = family;
  if (f == "conv_bf16x3" && n == 4)
    return a[0] >= 1 && a[0] < kBf16x3Tiles_n && bf16x3_supported(a[1], a[2])
               ? (int64_t)bf16x3_lds_bytes(a[0], a[1], a[2], a[3] != 0) : -1;
  if (f == "ups_bf16x3" && n == 1)
    return a[0] >= 0 && a[0] < kUpsCfgs_n ? (int64_t)ups_lds_bytes(a[0]) : -1;
  if (f == "resblock_bf16x3" && n == 3)
    return a[2] >= 1 && a[2] <= kRbMaxConv ? (int64_t)rb_lds_bytes(a[0], a[1], a[2]) : -1;
  if (f == "mrf_thin" && n == 1) return thin_window(a[0]) ? (int64_t)thin_lds_bytes(a[0]) : -1;
  if (f == "mrf_thin_mfma" && n == 1)
    return thin_mfma_window(a[0]) ? (int64_t)thin_mfma_lds_bytes(a[0]) : -1;
  if (f == "conv1d_mfma_f32" && n == 3)
    return a[0] >= 0 && a[0] < TILE_COUNT && fp32_conv_supported(a[0], a[1], a[2])
               ? (int64_t)fp32_conv_lds_bytes(a[0], a[1], a[2]) : -1;
  if (f == "conv_post" && n == 1) return a[0] >= 1 ? (int64_t)conv_post_lds_bytes(a[0]) : -1;
  if (f == "logmel_fft" && n == 4)
    return a[0] >= 16 && !(a[0] & (a[0] - 1)) && a[1] >= 1 && a[2] >= 1 && a[3] >= 1
               ? (int64_t)logmel_fft_lds_bytes(a[0], a[1], a[3], a[2]) : -1;
  // the DFT-GEMM pair (n_fft, hop): stft_power_mfma's tile where hfg_mel_create admits the pair
  if (f == "stft_power_mfma" && n == 2)
    return a[0] >= 1 && a[1] >= 1 && mel_dft_fits(a[0], a[1]) ? (int64_t)stft_lds_bytes(a[0], a[1])
                                                              : -1;
  return -1;
}

// The workspace layout of a forward (handle.h, WsLayout) as JSON: what the public sizes total
// and the schedule carves, for the host suite (tests/test_workspace_layout_host.py).
int hfg_debug_workspace(const hfg_handle* h, int64_t B, int64_t T_or_L, int taps, char* buf,
                        size_t buflen) {
  if (!h || !buf || buflen == 0) return fail(HFG_EINVAL, "bad arguments");
  if (B <= 0 || T_or_L <= 0) return fail(HFG_EINVAL, "B and T (L) must be > 0");
  if (B > kMaxBatch) return fail(HFG_EINVAL, "B must be in [1, 65535] (got %lld)", (long long)B);
  std::lock_guard<std::recursive_mutex> lk(const_cast<hfg_handle*>(h)->mu);
  const WsLayout lay = h->mrf_only ? mrf_ws_layout(h, B, T_or_L) : ws_layout(h, B, T_or_L, taps != 0);
  JsonWriter js;
  js.begin_object().integer("total", lay.total).key("parts").begin_array();
  for (int q = 0; q < lay.n_parts; ++q) {
    const WsPart& p = lay.part[q];
    js.begin_object().integer("b0", p.b0).integer("B", p.B).integer("off", p.off);
    js.integer("bytes", p.bytes).key("regions").begin_array();
    auto region = [&](const std::string& name, const WsRegion& r) {
      js.begin_object().string("name", name).integer("off", r.off).integer("bytes", r.bytes);
      js.end_object();
    };
    if (!h->mrf_only) region("X", p.X);
    region("R", p.rb.R), region("Tb", p.rb.Tb);
    if (!h->mrf_only) region("MRF", p.rb.out);
    for (int j = 0; p.conc && j < h->cfg.n_res; ++j) {
      const std::string rb = "rb" + std::to_string(j);
      region(rb + ".R", p.rb_conc[j].R), region(rb + ".Tb", p.rb_conc[j].Tb);
      region(rb + ".out", p.rb_conc[j].out);
    }
    if (!h->mrf_only) region("table", p.table);
    region("slots", p.slots);
    js.end_array().end_object();
  }
  js.end_array().end_object();
  return return_text(js.str(), buf, buflen);
}

// JSON description of everything the launch code reads from the plan (layers, whole-ResBlock
// and thin-stage launches, packed-buffer offsets) and the sha256 of the packed image: the
// fingerprint the host suite pins (tests/test_plan_host.py).  Commits pending weights first.
int hfg_debug_plan(hfg_handle* h, char* buf, size_t buflen) {
  if (!h || !buf || buflen == 0) return fail(HFG_EINVAL, "bad arguments");
  std::lock_guard<std::recursive_mutex> lk(h->mu);
  int rc = commit_if_dirty(h);
  if (rc) return rc;
  JsonWriter js;
  js.begin_object().key("layers").begin_array();
  for (const Layer& L : h->layers) {
    const Packing &pk = L.pk[0], &ps = L.pk[1];
    js.begin_object().string("mod", L.mod).integer("kind", L.kind).integer("prec", L.prec);
    js.integer("tile", pk.tile).integer("m_tiles", pk.m_tiles).integer("n_chunks", pk.n_chunks);
    js.integer("CK", L.CK).integer("ew", L.ew);
    js.integers("w", {(long long)pk.w.off, (long long)pk.w.len, (long long)pk.b.off, (long long)pk.b.len});
    js.integers("small", {ps.tile, ps.m_tiles, ps.n_chunks, (long long)ps.w.off, (long long)ps.b.off});
    js.integers("frames", {L.ups_cfg, L.m_tiles_f, (long long)L.wf.off, (long long)L.bf.off});
    js.end_object();
  }
  js.end_array().key("stages").begin_array();
  for (const Stage& st : h->stages) {
    js.begin_object().integer("C", st.C).integer("ups", st.conv_ups).integer("thin", st.thin);
    js.integer("thin_mfma", st.thin && st.thin_mfma);
    js.integers("conv1", st.conv1).integers("conv2", st.conv2);
    if (st.thin) {
      js.integers("thin_convs", st.thin_convs).integers("thin_conv0", st.thin_conv0);
      std::vector<size_t> w_off;
      for (const PackRegion& r : st.thin_w) w_off.push_back(r.off);
      js.integers("thin_halo", st.thin_halo).integers("thin_w_off", w_off);
      js.integer("thin_b_off", (long long)st.thin_b.off);
    }
    if (st.thin && st.thin_mfma) {
      js.integers("thin_m", {(long long)st.thin_m.off, (long long)(st.thin_m.len * sizeof(float))});
      js.integers("thin_m_conv", st.thin_m_conv);
    }
    js.key("rbs").begin_array();
    for (const RbFused& rb : st.rbs) {
      js.begin_object().integer("fused", rb.fused);
      if (rb.fused) {
        js.integers("convs", rb.convs).integer("kt", rb.kt).integer("nwin", rb.nwin);
        js.integer("wm", rb.wm).integer("halo", rb.halo).integer("W", rb.W);
        js.integer("split", rb.split);
        if (rb.split) js.integers("parts", {rb.halo_p[0], rb.halo_p[1], rb.W_p[0], rb.W_p[1]});
        js.integers("w", {(long long)rb.w.off, (long long)rb.w.len, (long long)rb.b.off, (long long)rb.b.len});
        js.integer("post", rb.post);  // conv_post fused into this launch, for a call that allows it
      }
      js.end_object();
    }
    js.end_array().end_object();
  }
  js.end_array().integer("packed_len", (long long)h->packed_host.size());
  js.string("sha256", sha256_hex(reinterpret_cast<const unsigned char*>(h->packed_host.data()),
                                 sizeof(float) * h->packed_host.size()));
  js.end_object();
  return return_text(js.str(), buf, buflen);
}

int hfg_forward_taps(hfg_handle* h, const float* mel, int64_t B, int64_t T, float* wav,
                     int64_t out_len, void* workspace, size_t workspace_bytes,
                     float* const* taps, int n_taps, void* stream) {
  int rc = check_generator(h);
  if (rc) return rc;
  if (!workspace) return fail(HFG_EINVAL, "workspace is NULL");
  if (taps && n_taps != 1 + 2 * h->cfg.n_up)
    return fail(HFG_EINVAL, "n_taps must be 1 + 2 * n_up = %d", 1 + 2 * h->cfg.n_up);
  ForwardScope scope(h);
  if ((rc = scope.ready(h))) return rc;
  return forward_run(h, FwdIo{mel, B, T, nullptr, wav, out_len, taps}, workspace, workspace_bytes,
                     reinterpret_cast<hipStream_t>(stream), true);
}

}  // extern "C"
