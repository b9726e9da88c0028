// disc_capi.cpp — C ABI of the discriminators (include/hifigan_hip_disc.h): one handle per
// PeriodDiscriminator / ScaleDiscriminator of the reference (models/hifigan.py:286-543), its
// layer table, shapes, weight store and launch schedule.  Kernels: disc_conv.hip (the middle
// layers on the matrix cores), disc_thin.hip (entry conv, conv_post, pooling, the
// feature-matching sums).
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "disc.h"
#include "frontend_host.h"

using namespace hfg_host;

namespace {

struct DiscLayer {
  int C_in, C_out, groups, k, stride, pad;
};
// PeriodDiscriminator.convs + conv_post (models/hifigan.py:484-493)
constexpr DiscLayer kPeriodLayers[] = {{1, 32, 1, 5, 3, 2},      {32, 128, 1, 5, 3, 2},
                                       {128, 512, 1, 5, 3, 2},   {512, 1024, 1, 5, 3, 2},
                                       {1024, 1024, 1, 5, 1, 2}, {1024, 1, 1, 3, 1, 1}};
// ScaleDiscriminator.convs + conv_post (models/hifigan.py:310-321)
constexpr DiscLayer kScaleLayers[] = {{1, 128, 1, 15, 1, 7},      {128, 128, 4, 41, 2, 20},
                                      {128, 256, 16, 41, 2, 20},  {256, 512, 16, 41, 4, 20},
                                      {512, 1024, 16, 41, 4, 20}, {1024, 1024, 16, 41, 1, 20},
                                      {1024, 1024, 1, 5, 1, 2},   {1024, 1, 1, 3, 1, 1}};
constexpr int64_t kDiscMaxT = (int64_t)1 << 28;

struct Param {
  std::vector<float> data;
  bool set = false;
};

}  // namespace

struct hfg_disc_handle {
  int kind, arg, device;
  std::vector<DiscLayer> layers;          // the last is conv_post
  std::map<std::string, Param> params;    // "<module>.weight" / "<module>.bias"
  std::vector<float> packed_host;         // every layer's operand and bias, 16-byte aligned
  std::vector<size_t> w_off, b_off;       // floats into packed_host / packed_dev
  std::vector<int> ew;                    // packing exponent of every matrix-core layer
  float* packed_dev = nullptr;
  bool committed = false;

  int n_maps() const { return (int)layers.size(); }
  std::string module(int i) const {
    return i + 1 == n_maps() ? std::string("conv_post") : "convs." + std::to_string(i);
  }
  int period() const { return kind == HFG_DISC_PERIOD ? arg : 1; }
  // the fold's rows (period) or the pooled length (scale); 0 if T is refused
  int64_t rows0(int64_t T) const {
    if (T < 1 || T > kDiscMaxT) return 0;
    if (kind == HFG_DISC_PERIOD) {
      const int64_t rem = T % arg;
      if (rem && arg - rem >= T) return 0;   // the reflect pad needs pad < T
      return (T + arg - 1) / arg;
    }
    int64_t L = T;
    for (int i = 0; i < arg; ++i) L = L / 2 + 1;
    return L;
  }
  // H of every map (H[0] = rows0: the entry conv's input)
  std::vector<int64_t> heights(int64_t T) const {
    std::vector<int64_t> H{rows0(T)};
    if (!H[0]) return {};
    for (const DiscLayer& L : layers) H.push_back((H.back() + 2 * L.pad - L.k) / L.stride + 1);
    return H;
  }
};

namespace {

size_t pool_floats(const hfg_disc_handle* h, int64_t B, int64_t T) {
  if (h->kind != HFG_DISC_SCALE) return 0;
  size_t n = 0;
  int64_t L = T;
  for (int i = 0; i < h->arg; ++i) {
    L = L / 2 + 1;
    n += (size_t)B * L;
  }
  return n;
}

int check_bt(const hfg_disc_handle* h, int64_t B, int64_t T) {
  if (B < 1 || B > 65535) return mfail(HFG_EINVAL, "B must be in [1, 65535]");
  if (T < 1 || T > kDiscMaxT)
    return mfail(HFG_EINVAL, "T must be in [1, %lld], got %lld", (long long)kDiscMaxT,
                 (long long)T);
  if (!h->rows0(T))
    return mfail(HFG_EINVAL, "period %d: the reflect pad of %lld samples does not fit T = %lld",
                 h->arg, (long long)(h->arg - T % h->arg), (long long)T);
  return HFG_OK;
}

}  // namespace

extern "C" {

int hfg_disc_create(int kind, int arg, int device, hfg_disc_handle** out) {
  if (!out) return mfail(HFG_EINVAL, "NULL argument");
  *out = nullptr;
  if (kind != HFG_DISC_PERIOD && kind != HFG_DISC_SCALE)
    return mfail(HFG_EINVAL, "discriminator kind must be HFG_DISC_PERIOD or HFG_DISC_SCALE");
  if (kind == HFG_DISC_PERIOD && (arg < 1 || arg > 65535))
    return mfail(HFG_EINVAL, "period must be in [1, 65535], got %d", arg);
  if (kind == HFG_DISC_SCALE && (arg < 0 || arg > 2))
    return mfail(HFG_EINVAL, "a scale discriminator has 0, 1 or 2 poolings, got %d", arg);
  if (device >= 0) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device >= n)
      return mfail(HFG_ENODEV, "no HIP device %d", device);
  }
  auto* h = new (std::nothrow) hfg_disc_handle();
  if (!h) return mfail(HFG_ENOMEM, "host alloc");
  h->kind = kind;
  h->arg = arg;
  h->device = device < 0 ? -1 : device;
  if (kind == HFG_DISC_PERIOD)
    h->layers.assign(std::begin(kPeriodLayers), std::end(kPeriodLayers));
  else
    h->layers.assign(std::begin(kScaleLayers), std::end(kScaleLayers));
  for (int i = 0; i < h->n_maps(); ++i) {
    h->params[h->module(i) + ".weight"];
    h->params[h->module(i) + ".bias"];
  }
  *out = h;
  return HFG_OK;
}

void hfg_disc_destroy(hfg_disc_handle* h) {
  if (!h) return;
  if (h->packed_dev) {
    DeviceGuard g(h->device);
    (void)hipFree(h->packed_dev);
  }
  delete h;
}

int hfg_disc_set_weight(hfg_disc_handle* h, const char* key, const float* data,
                        const int64_t* shape, int ndim) {
  if (!h || !key || !data || !shape) return mfail(HFG_EINVAL, "NULL argument");
  auto it = h->params.find(key);
  if (it == h->params.end()) return mfail(HFG_EINVAL, "unknown key '%s'", key);
  const std::string k(key);
  int li = 0;
  bool bias = false;
  for (int i = 0; i < h->n_maps(); ++i)
    if (k == h->module(i) + ".weight" || k == h->module(i) + ".bias")
      li = i, bias = k.back() == 's';
  const DiscLayer& L = h->layers[li];
  std::vector<int64_t> want;
  if (bias) {
    want = {L.C_out};
  } else {
    want = {L.C_out, L.C_in / L.groups, L.k};
    if (h->kind == HFG_DISC_PERIOD) want.push_back(1);
  }
  bool ok = ndim == (int)want.size();
  for (int d = 0; ok && d < ndim; ++d) ok = shape[d] == want[d];
  if (!ok) {
    std::string s;
    for (int64_t v : want) s += (s.empty() ? "" : ", ") + std::to_string(v);
    return mfail(HFG_EINVAL, "'%s': expected shape [%s]", key, s.c_str());
  }
  size_t n = 1;
  for (int64_t v : want) n *= (size_t)v;
  it->second.data.assign(data, data + n);
  it->second.set = true;
  h->committed = false;
  return HFG_OK;
}

int hfg_disc_commit(hfg_disc_handle* h) {
  if (!h) return mfail(HFG_EINVAL, "NULL argument");
  for (auto& kv : h->params)
    if (!kv.second.set) return mfail(HFG_EAGAIN, "weight '%s' was never set", kv.first.c_str());
  const int n = h->n_maps();
  h->w_off.assign(n, 0);
  h->b_off.assign(n, 0);
  h->ew.assign(n, 0);
  size_t at = 0;
  auto take = [&](size_t floats) {
    const size_t o = at;
    at += (floats + 3) / 4 * 4;
    return o;
  };
  for (int i = 0; i < n; ++i) {
    const DiscLayer& L = h->layers[i];
    const bool thin = i == 0 || i == n - 1;
    const int cig = L.C_in / L.groups, cog = L.C_out / L.groups;
    h->w_off[i] = take(thin ? (size_t)L.C_out * cig * L.k
                            : hfg::disc_conv_pack_floats(cig, cog, L.k, L.groups,
                                                         hfg::disc_conv_msub(cog)));
    h->b_off[i] = take(L.C_out);
  }
  h->packed_host.assign(at, 0.f);
  for (int i = 0; i < n; ++i) {
    const DiscLayer& L = h->layers[i];
    const std::vector<float>& w = h->params[h->module(i) + ".weight"].data;
    const std::vector<float>& b = h->params[h->module(i) + ".bias"].data;
    const int cig = L.C_in / L.groups, cog = L.C_out / L.groups;
    if (i == 0 || i == n - 1)
      std::copy(w.begin(), w.end(), h->packed_host.begin() + h->w_off[i]);
    else
      h->ew[i] = pack_disc_conv(
          w.data(), cig, cog, L.k, L.groups, hfg::disc_conv_msub(cog),
          reinterpret_cast<uint16_t*>(h->packed_host.data() + h->w_off[i]));
    std::copy(b.begin(), b.end(), h->packed_host.begin() + h->b_off[i]);
  }
  if (h->device >= 0) {
    DeviceGuard g(h->device);
    if (!g.ok) return mfail(HFG_ENODEV, "hipSetDevice(%d)", h->device);
    float* fresh = nullptr;
    if (hipMalloc(&fresh, at * sizeof(float)) != hipSuccess)
      return mfail(HFG_ENOMEM, "device alloc of %zu bytes", at * sizeof(float));
    if (hipMemcpy(fresh, h->packed_host.data(), at * sizeof(float), hipMemcpyHostToDevice) !=
        hipSuccess) {
      (void)hipFree(fresh);
      return mfail(HFG_EIO, "weight upload");
    }
    if (h->packed_dev) {
      // a forward in flight on any stream may still read the previous image
      (void)hipDeviceSynchronize();
      (void)hipFree(h->packed_dev);
    }
    h->packed_dev = fresh;
  }
  h->committed = true;
  return HFG_OK;
}

int hfg_disc_num_maps(const hfg_disc_handle* h) { return h ? h->n_maps() : -1; }

int hfg_disc_map_shape(const hfg_disc_handle* h, int64_t T, int i, int64_t dims[3]) {
  if (!h || !dims) return mfail(HFG_EINVAL, "NULL argument");
  if (i < 0 || i >= h->n_maps()) return mfail(HFG_EINVAL, "map index %d out of range", i);
  if (int rc = check_bt(h, 1, T)) return rc;
  const std::vector<int64_t> H = h->heights(T);
  dims[0] = h->layers[i].C_out;
  dims[1] = H[i + 1];
  dims[2] = h->period();
  return HFG_OK;
}

size_t hfg_disc_workspace_bytes(const hfg_disc_handle* h, int64_t B, int64_t T) {
  if (!h || B < 1 || B > 65535 || !h->rows0(T)) return 0;
  const size_t n = pool_floats(h, B, T) * sizeof(float);
  return n < 16 ? 16 : n;
}

int hfg_disc_forward(hfg_disc_handle* h, const float* wav, int64_t B, int64_t T,
                     float* const* maps, void* workspace, size_t workspace_bytes, void* stream) {
  if (!h || !wav || !maps || !workspace) return mfail(HFG_EINVAL, "NULL argument");
  const int n = h->n_maps();
  for (int i = 0; i < n; ++i)
    if (!maps[i]) return mfail(HFG_EINVAL, "NULL argument (maps[%d])", i);
  if (int rc = check_bt(h, B, T)) return rc;
  if (!h->committed) return mfail(HFG_EINVAL, "forward before hfg_disc_commit");
  const size_t need = hfg_disc_workspace_bytes(h, B, T);
  if (workspace_bytes < need)
    return mfail(HFG_EINVAL, "workspace too small (%zu < %zu bytes)", workspace_bytes, need);
  if (h->device < 0) return mfail(HFG_EINVAL, "host-only discriminator handle");
  DeviceGuard g(h->device);
  if (!g.ok) return mfail(HFG_ENODEV, "hipSetDevice(%d)", h->device);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const std::vector<int64_t> H = h->heights(T);
  const int W = h->period();
  const int batch = (int)B;

  // the entry conv's signal: the wave, or its pooling
  const float* src = wav;
  int64_t src_len = T;
  if (h->kind == HFG_DISC_SCALE) {
    float* dst = reinterpret_cast<float*>(workspace);
    for (int i = 0; i < h->arg; ++i) {
      if (hipError_t e = hfg::launch_disc_pool(src, src_len, dst, batch, s))
        return mfail(HFG_EIO, "pooling launch: %s", hipGetErrorString(e));
      src = dst;
      src_len = src_len / 2 + 1;
      dst += (size_t)B * src_len;
    }
  }
  const float* pd = h->packed_dev;
  {
    const DiscLayer& L = h->layers[0];
    hfg::DiscEntryParams p{src,    src_len,  maps[0],    pd + h->w_off[0], pd + h->b_off[0],
                           L.C_out, (int)H[0], W,         (int)H[1],        L.k,
                           L.stride, L.pad};
    if (hipError_t e = hfg::launch_disc_entry(p, batch, s))
      return mfail(HFG_EIO, "%s launch: %s", h->module(0).c_str(), hipGetErrorString(e));
  }
  for (int i = 1; i + 1 < n; ++i) {
    const DiscLayer& L = h->layers[i];
    hfg::DiscConvParams p{maps[i - 1],
                          maps[i],
                          reinterpret_cast<const __bf16*>(pd + h->w_off[i]),
                          pd + h->b_off[i],
                          L.C_in,
                          L.C_out,
                          L.groups,
                          (int)H[i],
                          W,
                          (int)H[i + 1],
                          L.k,
                          L.stride,
                          L.pad,
                          1,
                          h->ew[i]};
    if (hipError_t e = hfg::launch_disc_conv(p, batch, s, nullptr))
      return mfail(HFG_EIO, "%s launch: %s", h->module(i).c_str(), hipGetErrorString(e));
  }
  {
    const DiscLayer& L = h->layers[n - 1];
    if (hipError_t e = hfg::launch_disc_post(maps[n - 2], L.C_in, (int)H[n - 1], W,
                                             pd + h->w_off[n - 1], pd + h->b_off[n - 1],
                                             maps[n - 1], batch, s))
      return mfail(HFG_EIO, "conv_post launch: %s", hipGetErrorString(e));
  }
  return HFG_OK;
}

size_t hfg_disc_fm_workspace_bytes(const hfg_disc_handle* h, int64_t B) {
  if (!h || B < 1 || B > 65535) return 0;
  return hfg::disc_fm_workspace_bytes(B, h->n_maps());
}

int hfg_disc_fm_sums(hfg_disc_handle* h, int64_t B, int64_t T, const float* const* maps_real,
                     const float* const* maps_fake, double* sums, void* workspace,
                     size_t workspace_bytes, void* stream) {
  if (!h || !maps_real || !maps_fake || !sums || !workspace)
    return mfail(HFG_EINVAL, "NULL argument");
  const int n = h->n_maps();
  for (int i = 0; i < n; ++i)
    if (!maps_real[i] || !maps_fake[i]) return mfail(HFG_EINVAL, "NULL argument (map %d)", i);
  if (int rc = check_bt(h, B, T)) return rc;
  const size_t need = hfg_disc_fm_workspace_bytes(h, B);
  if (workspace_bytes < need)
    return mfail(HFG_EINVAL, "workspace too small (%zu < %zu bytes)", workspace_bytes, need);
  if (h->device < 0) return mfail(HFG_EINVAL, "host-only discriminator handle");
  DeviceGuard g(h->device);
  if (!g.ok) return mfail(HFG_ENODEV, "hipSetDevice(%d)", h->device);
  const std::vector<int64_t> H = h->heights(T);
  hfg::DiscFmArgs a{};
  a.n_maps = n;
  for (int i = 0; i < n; ++i) {
    a.real[i] = maps_real[i];
    a.fake[i] = maps_fake[i];
    a.n[i] = (int64_t)h->layers[i].C_out * H[i + 1] * h->period();
  }
  if (hipError_t e = hfg::launch_disc_fm_sums(a, (int)B, reinterpret_cast<double*>(workspace),
                                              sums, reinterpret_cast<hipStream_t>(stream)))
    return mfail(HFG_EIO, "feature-matching sums launch: %s", hipGetErrorString(e));
  return HFG_OK;
}

int hfg_disc_debug_unpacked(const hfg_disc_handle* h, int layer, int plane, float* out, size_t n) {
  if (!h || !out) return mfail(HFG_EINVAL, "NULL argument");
  if (!h->committed) return mfail(HFG_EINVAL, "no committed weights");
  if (layer < 1 || layer + 1 >= h->n_maps() || plane < 0 || plane > 1)
    return mfail(HFG_EINVAL, "layer %d / plane %d: not a packed layer", layer, plane);
  const DiscLayer& L = h->layers[layer];
  const int cig = L.C_in / L.groups, cog = L.C_out / L.groups;
  if (n != (size_t)L.C_out * cig * L.k)
    return mfail(HFG_EINVAL, "layer %d holds %zu weights", layer, (size_t)L.C_out * cig * L.k);
  std::memset(out, 0, n * sizeof(float));
  unpack_disc_conv(reinterpret_cast<const uint16_t*>(h->packed_host.data() + h->w_off[layer]), cig,
                   cog, L.k, L.groups, hfg::disc_conv_msub(cog), plane, h->ew[layer], out);
  return HFG_OK;
}

}  // extern "C"
