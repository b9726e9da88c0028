// hifigan_capi.cpp — the C ABI of libhifigan_hip.so (include/hifigan_hip.h and
// hifigan_hip_inspect.h): argument checks, the handle's lock and device, the parameter store
// keyed by the reference state_dict names with weight-norm folding, the error channel and the
// schedule-knob table.  The plan, the packers and the launch schedule are plan.cpp, pack.cpp
// and forward.cpp (handle.h).
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <tuple>

#include "handle.h"
#include "mel_kernels.h"

using namespace hfg_host;
using hfg::kTiles;

namespace {
thread_local std::string g_err;
std::mutex g_sched_mu;
std::map<std::string, int> g_sched;

const SchedKnob* sched_knob(const char* name) {
  if (!name) return nullptr;
  for (const SchedKnob& k : kSchedKnobs)
    if (!strcmp(k.name, name)) return &k;
  return nullptr;
}
}  // namespace

namespace hfg_host {
int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}
int hip_fail(hipError_t e, const char* what) {
  return fail(HFG_EIO, "%s: %s", what, hipGetErrorString(e));
}
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

namespace {
// what every generator forward entry refuses
int check_generator(const hfg_handle* h) {
  if (!h) return fail(HFG_EINVAL, "handle is NULL");
  if (h->device < 0) return fail(HFG_EINVAL, "host-only handle cannot run forward");
  if (h->mrf_only) return fail(HFG_EINVAL, "MRF-only handle: use hfg_mrf_forward");
  return HFG_OK;
}

int create_impl(const hfg_config* cfg, bool mrf_only, int device, hfg_handle** out) {
  if (!out) return fail(HFG_EINVAL, "out is NULL");
  *out = nullptr;
  int rc = validate_config(cfg);
  if (rc) return rc;
  if (device >= 0) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) return fail(HFG_ENODEV, "no HIP device available");
    if (device >= n) return fail(HFG_ENODEV, "device %d out of range (%d devices)", device, n);
  }
  hfg_handle* h = new (std::nothrow) hfg_handle();
  if (!h) return fail(HFG_ENOMEM, "out of host memory");
  h->cfg = *cfg;
  h->mrf_only = mrf_only;
  h->device = device;
  if (device >= 0) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess &&
        n > 0)
      h->n_cu = n;
  }
  rc = plan_handle(h);
  if (rc) {
    delete h;
    return rc;
  }
  *out = h;
  return HFG_OK;
}
}  // namespace

namespace {
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

// ============================================================================
// C ABI
// ============================================================================
extern "C" {

#ifndef HFG_SRC_HASH
#define HFG_SRC_HASH "unknown"
#endif
// "... src:<16 hex>": sha256 of the build inputs (csrc/, include/, flags), computed by
// build.py and compiled in, so a loaded binary can be matched to its source tree
const char* hfg_version(void) {
  return "hifigan_hip 0.4.0 gfx950 f16x3-mfma fp32-mfma bf16x3-mfma src:" HFG_SRC_HASH;
}

const char* hfg_last_error(void) { return g_err.c_str(); }

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

int hfg_create(const hfg_config* cfg, int device, hfg_handle** out) {
  return create_impl(cfg, false, device, out);
}

int hfg_mrf_create(const hfg_mrf_config* mc, int device, hfg_handle** out) {
  if (!out) return fail(HFG_EINVAL, "out is NULL");
  *out = nullptr;
  if (!mc) return fail(HFG_EINVAL, "config is NULL");
  if (mc->channels <= 0) return fail(HFG_EINVAL, "channels must be > 0");
  // the generator-level config of one MRF stage: validate_config checks the ResBlock lists
  hfg_config c{};
  c.n_mels = 1;
  c.n_up = 1;
  c.up_rates[0] = 1;
  c.up_kernels[0] = 1;
  c.c0 = 2 * mc->channels;
  c.n_res = mc->n_res;
  for (int j = 0; j < HFG_MAX_RES; ++j) {
    c.res_kernels[j] = mc->res_kernels[j];
    c.n_dil[j] = mc->n_dil[j];
    for (int m = 0; m < HFG_MAX_DIL; ++m) c.dil[j][m] = mc->dil[j][m];
  }
  c.dtype = mc->dtype;
  c.resblock_type = mc->resblock_type;
  return create_impl(&c, true, device, out);
}

void hfg_destroy(hfg_handle* h) {
  if (!h) return;
  {
    DeviceGuard g(h->device);
    if (h->device >= 0) {
      recycle_prof(h);
      for (auto e : h->event_pool) (void)hipEventDestroy(e);
      if (h->packed_dev) (void)hipFree(h->packed_dev);
      if (h->ws) (void)hipFree(h->ws);
      if (h->fork_ev) (void)hipEventDestroy(h->fork_ev);
      if (h->join_ev) (void)hipEventDestroy(h->join_ev);
      if (h->aux) (void)hipStreamDestroy(h->aux);
      for (int part = 0; part < 2; ++part) {
        if (h->rb_fork[part]) (void)hipEventDestroy(h->rb_fork[part]);
        for (int j = 0; j < HFG_MAX_RES; ++j) {
          if (h->rb_join[part][j]) (void)hipEventDestroy(h->rb_join[part][j]);
          if (h->rb_aux[part][j]) (void)hipStreamDestroy(h->rb_aux[part][j]);
        }
      }
    }
  }
  delete h;
}

int hfg_num_params(const hfg_handle* h) { return h ? (int)h->param_order.size() : 0; }

int hfg_set_weight(hfg_handle* h, const char* name, const void* data, const int64_t* shape,
                   int ndim, int is_device) {
  if (!h || !name || !data || (!shape && ndim > 0))
    return fail(HFG_EINVAL, "NULL argument to hfg_set_weight");
  std::lock_guard<std::recursive_mutex> lk(h->mu);
  std::string key(name);
  std::vector<int64_t> shp(shape, shape + ndim);
  size_t n = 1;
  for (auto d : shp) {
    if (d < 0) return fail(HFG_EINVAL, "negative dimension for '%s'", name);
    n *= (size_t)d;
  }
  std::vector<float> buf(n);
  if (is_device) {
    if (h->device < 0) return fail(HFG_EINVAL, "device pointer given to a host-only handle");
    DeviceGuard g(h->device);
    hipError_t e = hipMemcpy(buf.data(), data, n * sizeof(float), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(e, "hipMemcpy(set_weight)");
  } else {
    std::memcpy(buf.data(), data, n * sizeof(float));
  }
  auto ends_with = [&](const char* suf) {
    size_t l = strlen(suf);
    return key.size() > l && key.compare(key.size() - l, l, suf) == 0;
  };
  // a ResBlock key of the other block type: say which layout this handle holds
  const bool pair_key = key.find(".convs1.") != std::string::npos ||
                        key.find(".convs2.") != std::string::npos;
  if (h->cfg.resblock_type == 1 && pair_key)
    return fail(HFG_EINVAL, "key '%s': this handle holds ResBlock2 blocks (resblock_type 1), whose "
                "parameters are resblocks.{j}.convs.{m}.*, not convs1 / convs2", name);
  if (h->cfg.resblock_type == 0 && key.find(".convs.") != std::string::npos)
    return fail(HFG_EINVAL, "key '%s': this handle holds the reference's ResBlock (resblock_type "
                "0), whose parameters are resblocks.{j}.convs1.{m}.* / convs2.{m}.*; create it "
                "with resblock_type 1 for ResBlock2's convs.{m}", name);
  if (ends_with(".weight_g") || ends_with(".weight_v")) {
    // apply_weight_norm layout (models/hifigan.py:274-283): w = g * v / ||v||, dim=0
    const std::string mod = key.substr(0, key.size() - 9);
    auto it = h->params.find(mod + ".weight");
    if (it == h->params.end()) return fail(HFG_EINVAL, "unknown key '%s'", name);
    const auto& wshape = it->second.shape;
    if (ends_with(".weight_v")) {
      if (shp != wshape) return fail(HFG_EINVAL, "shape mismatch for '%s'", name);
    } else {
      std::vector<int64_t> gshape(wshape.size(), 1);
      gshape[0] = wshape[0];
      if (shp != gshape) return fail(HFG_EINVAL, "shape mismatch for '%s'", name);
    }
    Param& part = h->wn_parts[key];
    part.shape = shp;
    part.data = std::move(buf);
    part.set = true;
    auto g = h->wn_parts.find(mod + ".weight_g");
    auto v = h->wn_parts.find(mod + ".weight_v");
    if (g != h->wn_parts.end() && v != h->wn_parts.end() && g->second.set && v->second.set) {
      Param& W = it->second;
      const size_t d0 = (size_t)wshape[0];
      const size_t inner = v->second.data.size() / d0;
      W.data.resize(v->second.data.size());
      for (size_t i = 0; i < d0; ++i) {
        double ss = 0.0;
        const float* vv = v->second.data.data() + i * inner;
        for (size_t q = 0; q < inner; ++q) ss += (double)vv[q] * vv[q];
        const double scale = (double)g->second.data[i] / std::sqrt(ss);
        for (size_t q = 0; q < inner; ++q) W.data[i * inner + q] = (float)(vv[q] * scale);
      }
      W.set = true;
      h->dirty = true;
    }
    return HFG_OK;
  }
  auto it = h->params.find(key);
  if (it == h->params.end()) return fail(HFG_EINVAL, "unknown key '%s'", name);
  if (shp != it->second.shape) {
    std::string want;
    for (auto d : it->second.shape) want += std::to_string(d) + ",";
    return fail(HFG_EINVAL, "shape mismatch for '%s' (expected [%s])", name, want.c_str());
  }
  it->second.data = std::move(buf);
  it->second.set = true;
  h->dirty = true;
  return HFG_OK;
}

int hfg_commit_weights(hfg_handle* h) {
  if (!h) return fail(HFG_EINVAL, "handle is NULL");
  std::lock_guard<std::recursive_mutex> lk(h->mu);
  return do_commit(h);
}

int64_t hfg_out_len(const hfg_handle* h, int64_t T) {
  if (!h || T <= 0 || h->mrf_only) return -1;
  return shapes_for(h, T).L.back();
}

size_t hfg_workspace_bytes(const hfg_handle* h, int64_t B, int64_t T) {
  if (!h || B <= 0 || T <= 0 || h->mrf_only) return 0;
  return ws_bytes_for(h, B, T);
}

int hfg_reserve(hfg_handle* h, int64_t B, int64_t T) {
  if (!h) return fail(HFG_EINVAL, "handle is NULL");
  if (h->mrf_only) return fail(HFG_EINVAL, "MRF-only handle has no generator workspace");
  std::lock_guard<std::recursive_mutex> lk(h->mu);
  if (h->device < 0) return fail(HFG_EINVAL, "host-only handle");
  if (B <= 0 || T <= 0) return fail(HFG_EINVAL, "B and T must be > 0");
  const size_t need = ws_bytes_for(h, B, T);
  if (need <= h->ws_bytes) return HFG_OK;
  DeviceGuard g(h->device);
  if (!g.ok) return fail(HFG_ENODEV, "hipSetDevice(%d) failed", h->device);
  if (h->ws) {
    (void)hipDeviceSynchronize();
    (void)hipFree(h->ws);
  }
  h->ws = nullptr;
  h->ws_bytes = 0;
  hipError_t e = hipMalloc(&h->ws, need);
  if (e != hipSuccess) return fail(HFG_ENOMEM, "hipMalloc(workspace %zu B): %s", need,
                                   hipGetErrorString(e));
  h->ws_bytes = need;
  return HFG_OK;
}

int hfg_forward_ex(hfg_handle* h, const float* mel, int64_t B, int64_t T,
                   const hfg_forward_opts* opts, float* wav, int64_t out_len, void* workspace,
                   size_t workspace_bytes, void* stream) {
  int rc = check_generator(h);
  if (rc) return rc;
  ForwardScope scope(h);
  if (!workspace) return fail(HFG_EINVAL, "workspace is NULL");
  if ((rc = scope.ready(h))) return rc;
  return forward_run(h, FwdIo{mel, B, T, opts, wav, out_len, nullptr}, workspace, workspace_bytes,
                     reinterpret_cast<hipStream_t>(stream), false);
}

int hfg_forward_ws(hfg_handle* h, const float* mel, int64_t B, int64_t T, float* wav,
                   int64_t out_len, void* workspace, size_t workspace_bytes, void* stream) {
  return hfg_forward_ex(h, mel, B, T, nullptr, wav, out_len, workspace, workspace_bytes, stream);
}

int hfg_forward(hfg_handle* h, const float* mel, int64_t B, int64_t T, float* wav,
                int64_t out_len, void* stream) {
  int rc = check_generator(h);
  if (rc) return rc;
  std::lock_guard<std::recursive_mutex> lk(h->mu);
  if ((rc = hfg_reserve(h, B, T))) return rc;
  return hfg_forward_ws(h, mel, B, T, wav, out_len, h->ws, h->ws_bytes, stream);
}

// ---- one MRF / one ResBlock (MRF-only handles, hfg_mrf_create) ---------------
namespace {
int mrf_entry(hfg_handle* h, int only_j, const float* x, int64_t B, int64_t L, float* y, void* ws,
              size_t ws_bytes, void* stream) {
  if (!h) return fail(HFG_EINVAL, "handle is NULL");
  if (!h->mrf_only) return fail(HFG_EINVAL, "not an MRF handle (hfg_mrf_create)");
  if (h->device < 0) return fail(HFG_EINVAL, "host-only handle cannot run forward");
  if (!x || !y || !ws) return fail(HFG_EINVAL, "x / y / workspace pointer is NULL");
  if (x == y) return fail(HFG_EINVAL, "y must not alias x");
  if (B <= 0 || L <= 0) return fail(HFG_EINVAL, "B and L must be > 0");
  if ((int64_t)h->stages[0].C * L >= ((int64_t)1 << 30))
    return fail(HFG_EINVAL, "per-item activation reaches 2^30 elements");
  ForwardScope scope(h);
  const WsLayout lay = mrf_ws_layout(h, B, L);
  if (ws_bytes < lay.total) return fail(HFG_EINVAL, "workspace too small");
  int rc = scope.ready(h);
  if (rc) return rc;
  return mrf_run(h, only_j, x, L, y, lay.part[0], ws, reinterpret_cast<hipStream_t>(stream));
}
}  // namespace

size_t hfg_mrf_workspace_bytes(const hfg_handle* h, int64_t B, int64_t L) {
  if (!h || !h->mrf_only || B <= 0 || L <= 0) return 0;
  return mrf_ws_layout(h, B, L).total;
}

int hfg_mrf_forward(hfg_handle* h, const float* x, int64_t B, int64_t L, float* y,
                    void* workspace, size_t workspace_bytes, void* stream) {
  return mrf_entry(h, -1, x, B, L, y, workspace, workspace_bytes, stream);
}

int hfg_resblock_forward(hfg_handle* h, int j, const float* x, int64_t B, int64_t L, float* y,
                         void* workspace, size_t workspace_bytes, void* stream) {
  if (h && (j < 0 || j >= h->cfg.n_res)) return fail(HFG_EINVAL, "resblock index %d out of range", j);
  return mrf_entry(h, j, x, B, L, y, workspace, workspace_bytes, stream);
}

// ---- content hash of parameter tensors -----------------------------------------
int hfg_checksum32(const void* const* ptrs, const int64_t* nbytes, int n, uint32_t* out,
                   void* stream) {
  if (n < 0 || (n > 0 && (!ptrs || !nbytes || !out))) return fail(HFG_EINVAL, "bad arguments");
  if (n == 0) return HFG_OK;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipError_t e = hipMemsetAsync(out, 0, sizeof(uint32_t) * (size_t)n, st);
  if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync(checksum)");
  for (int base = 0; base < n; base += hfg::kChecksumMax) {
    hfg::ChecksumArgs a{};
    a.base = base;
    a.count = std::min(hfg::kChecksumMax, n - base);
    for (int i = 0; i < a.count; ++i) {
      if (nbytes[base + i] % 4 != 0 || (nbytes[base + i] > 0 && !ptrs[base + i]))
        return fail(HFG_EINVAL, "tensor %d: size must be a multiple of 4 bytes", base + i);
      a.p[i] = static_cast<const uint32_t*>(ptrs[base + i]);
      a.n[i] = nbytes[base + i] / 4;
    }
    e = hfg::launch_checksum(a, out, st);
    if (e != hipSuccess) return hip_fail(e, "launch checksum");
  }
  return HFG_OK;
}

int hfg_set_streams(hfg_handle* h, int n) {
  if (!h) return fail(HFG_EINVAL, "handle is NULL");
  std::lock_guard<std::recursive_mutex> lk(h->mu);
  if (n != 1 && n != 2) return fail(HFG_EINVAL, "streams must be 1 or 2 (got %d)", n);
  h->split = n;
  return HFG_OK;
}

int hfg_set_profiling(hfg_handle* h, int enable) {
  if (!h) return fail(HFG_EINVAL, "handle is NULL");
  std::lock_guard<std::recursive_mutex> lk(h->mu);
  h->profiling = enable != 0;
  return HFG_OK;
}

int hfg_profile_reset(hfg_handle* h) {
  if (!h) return fail(HFG_EINVAL, "handle is NULL");
  std::lock_guard<std::recursive_mutex> lk(h->mu);
  DeviceGuard g(h->device);
  for (auto& r : h->prof)
    if (r.e1) (void)hipEventSynchronize(r.e1);
  recycle_prof(h);
  return HFG_OK;
}

int hfg_profile_summary(hfg_handle* h, char* buf, size_t buflen) {
  if (!h || !buf || buflen == 0) return fail(HFG_EINVAL, "bad arguments");
  std::lock_guard<std::recursive_mutex> lk(h->mu);
  DeviceGuard g(h->device);
  struct Agg {
    int launches = 0;
    double ms = 0, flop = 0, bytes = 0;
  };
  std::map<std::string, Agg> agg;
  // a split forward's two half-batch dispatches of one layer count as one launch: its
  // FLOP / bytes summed over the halves, its time the union of the two intervals
  std::map<std::tuple<int, int>, std::pair<const ProfRec*, const ProfRec*>> pairs;
  for (auto& r : h->prof) {
    if (!r.e0 || !r.e1 || !r.label) continue;
    auto& pr = pairs[std::make_tuple(r.fwd, r.seq)];
    (r.part == 0 ? pr.first : pr.second) = &r;
  }
  auto elapsed = [](hipEvent_t a, hipEvent_t b, float* ms) -> hipError_t {
    hipError_t e = hipEventSynchronize(b);
    if (e == hipSuccess) e = hipEventSynchronize(a);
    if (e == hipSuccess) e = hipEventElapsedTime(ms, a, b);
    return e;
  };
  for (auto& kv : pairs) {
    const ProfRec* A = kv.second.first ? kv.second.first : kv.second.second;
    const ProfRec* Bq = kv.second.first ? kv.second.second : nullptr;
    float dA = 0.f;
    hipError_t e = elapsed(A->e0, A->e1, &dA);
    if (e != hipSuccess) return hip_fail(e, "hipEventElapsedTime");
    double ms = dA, flop = A->flop, bytes = A->bytes;
    if (Bq) {
      // B's start / end relative to A's start (either order)
      float s0 = 0.f, s1 = 0.f;
      if (elapsed(A->e0, Bq->e0, &s0) != hipSuccess || s0 < 0.f) {
        float r = 0.f;
        if (elapsed(Bq->e0, A->e0, &r) != hipSuccess) return fail(HFG_EIO, "event order");
        s0 = -r;
      }
      float dB = 0.f;
      e = elapsed(Bq->e0, Bq->e1, &dB);
      if (e != hipSuccess) return hip_fail(e, "hipEventElapsedTime");
      s1 = s0 + dB;
      ms = std::max<double>(dA, s1) - std::min<double>(0.0, s0);
      flop += Bq->flop;
      bytes += Bq->bytes;
    }
    Agg& a = agg[A->label];
    a.launches++;
    a.ms += ms;
    a.flop += flop;
    a.bytes += bytes;
  }
  std::string s = "{";
  bool first = true;
  for (auto& kv : agg) {
    char line[512];
    snprintf(line, sizeof(line), "%s\"%s\": {\"launches\": %d, \"ms\": %.6f, \"flop\": %.6e, "
             "\"bytes\": %.6e}", first ? "" : ", ", kv.first.c_str(), kv.second.launches,
             kv.second.ms, kv.second.flop, kv.second.bytes);
    s += line;
    first = false;
  }
  s += "}";
  if (s.size() + 1 > buflen) return fail(HFG_EINVAL, "buffer too small (%zu needed)", s.size() + 1);
  memcpy(buf, s.c_str(), s.size() + 1);
  return HFG_OK;
}

// ---- inspection helpers (not part of the public header's compute API) ------
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
  for (auto& L : h->layers) {
    if (L.mod != name) continue;
    if (which == 2) {
      if (L.ups_cfg < 0) return fail(HFG_EINVAL, "%s has no output-frame packing", name.c_str());
      const hfg::UpsCfg& tf = hfg::kUpsCfgs[L.ups_cfg];
      const size_t w_len = (size_t)L.m_tiles_f * (L.C_in / 16) * 8 * tf.MT() * 16 / 2;
      const size_t b_len = (size_t)L.C_out;
      if (info) {
        const int64_t v[10] = {L.kind, (int64_t)L.C_out * L.s / 2, 2, L.ups_cfg, L.m_tiles_f,
                               L.C_in / 16, (int64_t)w_len, (int64_t)b_len, 16, tf.MT()};
        std::copy_n(v, 10, info);
      }
      if (!out) return HFG_OK;
      if (h->dirty) {
        int rc = do_commit(h);
        if (rc) return rc;
      }
      if (cap < w_len + b_len) return fail(HFG_EINVAL, "output buffer too small");
      memcpy(out, h->packed_host.data() + L.wf_off, sizeof(float) * w_len);
      memcpy(out + w_len, h->packed_host.data() + L.bf_off, sizeof(float) * b_len);
      return HFG_OK;
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
      info[6] = (int64_t)pk.w_len;
      info[7] = (int64_t)pk.b_len;
      info[8] = L.CK;
      info[9] = L.kind == L_POST ? 0
                : L.prec == 1    ? hfg::kBf16x3Tiles[pk.tile].MT()
                                 : kTiles[pk.tile].MT();
    }
    if (!out) return HFG_OK;
    if (h->dirty) {
      int rc = do_commit(h);
      if (rc) return rc;
    }
    if (cap < pk.w_len + pk.b_len) return fail(HFG_EINVAL, "output buffer too small");
    memcpy(out, h->packed_host.data() + pk.w_off, sizeof(float) * pk.w_len);
    memcpy(out + pk.w_len, h->packed_host.data() + pk.b_off, sizeof(float) * pk.b_len);
    return HFG_OK;
  }
  return fail(HFG_EINVAL, "unknown layer '%s'", mod);
}

// The f16x3 packing exponent of layer `mod` (0 in the other modes): set by the commit, so a
// handle with uncommitted weights commits first and returns its error (e.g. weights missing).
int hfg_debug_layer_exponent(hfg_handle* h, const char* mod, int* ew) {
  if (!h || !mod || !ew) return fail(HFG_EINVAL, "NULL argument");
  for (auto& L : h->layers) {
    if (L.mod != mod) continue;
    if (h->dirty) {
      int rc = do_commit(h);
      if (rc) return rc;
    }
    *ew = L.ew;
    return HFG_OK;
  }
  return fail(HFG_EINVAL, "unknown layer '%s'", mod);
}

int hfg_debug_packed_resblock(hfg_handle* h, int stage, int j, float* out, size_t cap,
                              int64_t* info) {
  if (!h || !info) return fail(HFG_EINVAL, "NULL argument");
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
  info[6] = (int64_t)rb.w_len;
  info[7] = (int64_t)rb.b_len;
  if (!out) return HFG_OK;
  if (h->dirty) {
    int rc = do_commit(h);
    if (rc) return rc;
  }
  if (cap < rb.w_len + rb.b_len) return fail(HFG_EINVAL, "output buffer too small");
  memcpy(out, h->packed_host.data() + rb.w_off, sizeof(float) * rb.w_len);
  memcpy(out + rb.w_len, h->packed_host.data() + rb.b_off, sizeof(float) * rb.b_len);
  return HFG_OK;
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
  const WsLayout lay = h->mrf_only ? mrf_ws_layout(h, B, T_or_L) : ws_layout(h, B, T_or_L, taps != 0);
  std::string s = "{\"total\": " + std::to_string(lay.total) + ", \"parts\": [";
  for (int q = 0; q < lay.n_parts; ++q) {
    const WsPart& p = lay.part[q];
    s += std::string(q ? ", " : "") + "{\"b0\": " + std::to_string(p.b0) + ", \"B\": " +
         std::to_string(p.B) + ", \"off\": " + std::to_string(p.off) + ", \"bytes\": " +
         std::to_string(p.bytes) + ", \"regions\": [";
    bool first = true;
    auto region = [&](const std::string& name, const WsRegion& r) {
      s += std::string(first ? "" : ", ") + "{\"name\": \"" + name + "\", \"off\": " +
           std::to_string(r.off) + ", \"bytes\": " + std::to_string(r.bytes) + "}";
      first = false;
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
    s += "]}";
  }
  s += "]}";
  if (s.size() + 1 > buflen) return fail(HFG_EINVAL, "buffer too small (%zu needed)", s.size() + 1);
  memcpy(buf, s.c_str(), s.size() + 1);
  return HFG_OK;
}

// JSON description of everything the launch code reads from the plan (layers, whole-ResBlock
// and thin-stage launches, packed-buffer offsets) and the sha256 of the packed image: the
// fingerprint the host suite pins (tests/test_plan_host.py).  Commits pending weights first.
int hfg_debug_plan(hfg_handle* h, char* buf, size_t buflen) {
  if (!h || !buf || buflen == 0) return fail(HFG_EINVAL, "bad arguments");
  std::lock_guard<std::recursive_mutex> lk(h->mu);
  if (h->dirty) {
    int rc = do_commit(h);
    if (rc) return rc;
  }
  std::string s;
  auto num = [&](const char* key, long long v) { s += "\"" + std::string(key) + "\": " + std::to_string(v) + ", "; };
  auto list = [&](const char* key, std::initializer_list<long long> v) {
    s += "\"" + std::string(key) + "\": [";
    for (long long x : v) s += std::to_string(x) + ",";
    s += "], ";
  };
  auto vec = [&](const char* key, const auto& v) {
    s += "\"" + std::string(key) + "\": [";
    for (auto x : v) s += std::to_string((long long)x) + ",";
    s += "], ";
  };
  s = "{\"layers\": [";
  for (const Layer& L : h->layers) {
    s += "{\"mod\": \"" + L.mod + "\", ";
    const Packing &pk = L.pk[0], &ps = L.pk[1];
    num("kind", L.kind), num("prec", L.prec), num("tile", pk.tile), num("m_tiles", pk.m_tiles);
    num("n_chunks", pk.n_chunks), num("CK", L.CK), num("ew", L.ew);
    list("w", {(long long)pk.w_off, (long long)pk.w_len, (long long)pk.b_off, (long long)pk.b_len});
    list("small", {ps.tile, ps.m_tiles, ps.n_chunks, (long long)ps.w_off, (long long)ps.b_off});
    list("frames", {L.ups_cfg, L.m_tiles_f, (long long)L.wf_off, (long long)L.bf_off});
    s += "}, ";
  }
  s += "], \"stages\": [";
  for (size_t i = 0; i < h->stages.size(); ++i) {
    const Stage& st = h->stages[i];
    s += "{";
    num("C", st.C), num("ups", st.conv_ups), num("thin", st.thin), num("thin_mfma", st.thin && st.thin_mfma);
    vec("conv1", st.conv1), vec("conv2", st.conv2);
    if (st.thin) {
      vec("thin_convs", st.thin_convs), vec("thin_conv0", st.thin_conv0), vec("thin_halo", st.thin_halo);
      vec("thin_w_off", st.thin_w_off), num("thin_b_off", (long long)st.thin_b_off);
    }
    if (st.thin && st.thin_mfma) {
      list("thin_m", {(long long)st.thin_m_off, (long long)st.thin_m_bytes});
      vec("thin_m_conv", st.thin_m_conv);
    }
    s += "\"rbs\": [";
    for (size_t j = 0; j < st.rbs.size(); ++j) {
      const RbFused& rb = st.rbs[j];
      s += "{";
      num("fused", rb.fused);
      if (rb.fused) {
        vec("convs", rb.convs);
        num("kt", rb.kt), num("nwin", rb.nwin), num("wm", rb.wm), num("halo", rb.halo), num("W", rb.W);
        num("split", rb.split);
        if (rb.split) list("parts", {rb.halo_p[0], rb.halo_p[1], rb.W_p[0], rb.W_p[1]});
        list("w", {(long long)rb.w_off, (long long)rb.w_len, (long long)rb.b_off, (long long)rb.b_len});
        num("post", rb.post);  // conv_post fused into this launch, for a call that allows it
      }
      s += "}, ";
    }
    s += "]}, ";
  }
  s += "], ";
  num("packed_len", (long long)h->packed_host.size());
  s += "\"sha256\": \"" + sha256_hex(reinterpret_cast<const unsigned char*>(h->packed_host.data()),
                                     sizeof(float) * h->packed_host.size()) + "\"}";
  // the appenders end every item with a separator: drop the one in front of a closing bracket
  size_t n = 0;
  for (char ch : s) {
    if (ch == ']' || ch == '}')
      while (s[n - 1] == ' ' || s[n - 1] == ',') --n;
    s[n++] = ch;
  }
  s.resize(n);
  if (s.size() + 1 > buflen) return fail(HFG_EINVAL, "buffer too small (%zu needed)", s.size() + 1);
  memcpy(buf, s.c_str(), s.size() + 1);
  return HFG_OK;
}

int hfg_forward_taps(hfg_handle* h, const float* mel, int64_t B, int64_t T, float* wav,
                     int64_t out_len, void* workspace, size_t workspace_bytes,
                     float* const* taps, int n_taps, void* stream) {
  if (!h) return fail(HFG_EINVAL, "handle is NULL");
  if (h->device < 0 || h->mrf_only) return fail(HFG_EINVAL, "not a generator device handle");
  if (!workspace) return fail(HFG_EINVAL, "workspace is NULL");
  if (taps && n_taps != 1 + 2 * h->cfg.n_up)
    return fail(HFG_EINVAL, "n_taps must be 1 + 2 * n_up = %d", 1 + 2 * h->cfg.n_up);
  ForwardScope scope(h);
  int rc = scope.ready(h);
  if (rc) return rc;
  return forward_run(h, FwdIo{mel, B, T, nullptr, wav, out_len, taps}, workspace, workspace_bytes,
                     reinterpret_cast<hipStream_t>(stream), true);
}

}  // extern "C"
