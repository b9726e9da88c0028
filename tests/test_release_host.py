"""The public HiFi-GAN release's Generator on the CPU container: ResBlock2 (config
"resblock": "2", generator V3) and the release's final leaky_relu slope 0.01, through the
constructors, the config structs, checkpoint loading, the whole-ResBlock2 packing
(resblock2_bf16x3's A stream and windowing, emulated in numpy) and the receptive field.
Handles are host-only (device = -1): no test here needs a GPU."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

from oracle import config as C, hifigan_torch as H, prng
from release_oracle import release_forward
from test_capi_host import SPLIT_TOL, _conv_same, _lrelu, dec

V3_JSON = {"resblock": "2", "upsample_rates": [8, 8, 4], "upsample_kernel_sizes": [16, 16, 8],
           "upsample_initial_channel": 256, "resblock_kernel_sizes": [3, 5, 7],
           "resblock_dilation_sizes": [[1, 2], [2, 6], [3, 12]], "num_mels": 80}


@pytest.fixture(scope="module")
def S(pkg):
    import __graft_entry__ as ge
    return importlib.import_module(ge.PKG_NAME + ".synth")


@pytest.fixture(scope="module")
def ckpt(pkg):
    import __graft_entry__ as ge
    return importlib.import_module(ge.PKG_NAME + ".checkpoint")


def test_restatement_equals_the_reference_oracle_for_type_1():
    """release_forward with resblock "1" and slope 0.1 is oracle.hifigan_torch's op
    sequence: bitwise the same wav (float32, CPU)."""
    for cfg, seed in ((C.V2STAR, 5), (C.NONEXACT, 6)):
        sd = C.make_state_dict(cfg, seed=seed)
        mel = torch.from_numpy(prng.mel_input(seed, (2, cfg.n_mels, 9)))
        ref = H.generator_forward(H.to_torch_state(sd), cfg, mel)
        assert torch.equal(release_forward(sd, cfg, mel), ref)


def test_constructor_defaults_are_todays_generator(pkg):
    gen = pkg.HiFiGANGenerator()
    assert list(gen.state_dict()) == [k for k, _, _ in C.param_specs(C.V1)]
    assert len(gen.state_dict()) == 156
    assert gen.resblock == "1" and gen.final_lrelu_slope == 0.1
    # the struct's tail stays zero: the handle is the one every earlier caller got
    assert gen._hfg_cfg.resblock_type == 0 and gen._hfg_cfg.post_slope == 0.0
    assert pkg.load_library().hfg_num_params(pkg.Handle(gen._hfg_cfg, -1).ptr) == 156


def test_resblock2_constructors_and_weight_norm(pkg, S):
    cfg = S.RELEASE_V3
    gen = pkg.HiFiGANGenerator(**cfg.kwargs())
    specs = S.param_specs(cfg)
    assert [k for k, _, _ in specs] == list(gen.state_dict())
    for k, shape, _ in specs:
        assert tuple(gen.state_dict()[k].shape) == shape, k
    assert "mrfs.2.resblocks.2.convs.1.weight" in gen.state_dict()
    assert gen.state_dict()["mrfs.2.resblocks.2.convs.1.weight"].shape == (32, 32, 7)
    assert not any("convs1" in k or "convs2" in k for k in gen.state_dict())
    assert isinstance(gen.mrfs[0].resblocks[0], pkg.ResBlock2)
    assert gen.mrfs[2].resblocks[2].convs[1].dilation == (12,)
    assert gen.mrfs[2].resblocks[2].convs[1].padding == (36,)
    # the handle's key space is the module's
    h = pkg.Handle(gen._hfg_cfg, -1)
    assert pkg.load_library().hfg_num_params(h.ptr) == len(gen.state_dict())
    for k, t in gen._hip_weight_items():
        h.set_weight(k, t)
    h.commit()
    gen.apply_weight_norm()
    keys = list(gen.state_dict())
    assert "mrfs.0.resblocks.1.convs.0.weight_g" in keys
    assert "mrfs.0.resblocks.1.convs.0.weight_v" in keys
    assert "mrfs.0.resblocks.1.convs.0.weight" not in keys
    assert "ups.0.weight_g" in keys and "conv_pre.weight" in keys
    h2 = pkg.Handle(gen._hfg_cfg, -1)
    for k, t in gen._hip_weight_items():
        h2.set_weight(k, t)
    h2.commit()
    gen.remove_weight_norm()  # (torch re-registers weight after bias: compare as sets)
    assert set(gen.state_dict()) == {k for k, _, _ in specs}
    # the standalone block and MRF
    rb = pkg.ResBlock2(32, 7, (3, 12))
    assert list(rb.state_dict()) == ["convs.0.weight", "convs.0.bias", "convs.1.weight",
                                     "convs.1.bias"]
    assert [k for k, _ in rb._hip_weight_items()] == ["resblocks.0." + k for k in rb.state_dict()]
    mrf = pkg.MRF(64, [3, 5], [[1, 2], [2, 6]], resblock="2")
    assert len(mrf.state_dict()) == 8 and isinstance(mrf.resblocks[1], pkg.ResBlock2)
    hm = mrf._hip_new_handle(-1)
    for k, t in mrf._hip_weight_items():
        hm.set_weight(k, t)
    hm.commit()
    with pytest.raises(ValueError):
        pkg.MRF(64, resblock="3")


def test_config_structs_and_validation(pkg):
    lib = pkg.load_library()
    args = (80, [8, 8, 4], [16, 16, 8], 256, [3, 5, 7], [[1, 2], [2, 6], [3, 12]])
    c = pkg.make_config(*args, resblock="2", final_lrelu_slope=0.01)
    assert c.resblock_type == 1 and c.post_slope == np.float32(0.01)
    d = pkg.make_config(*args)
    assert d.resblock_type == 0 and d.post_slope == 0.0
    assert pkg.make_config(*args, final_lrelu_slope=0.1).post_slope == 0.0
    m = pkg._lib.make_mrf_config(32, [7], [[3, 12]], "f16x3", resblock="2")
    assert m.resblock_type == 1
    assert pkg._lib.make_mrf_config(32, [7], [[3, 12]]).resblock_type == 0
    h = ctypes.c_void_p()
    assert lib.hfg_create(ctypes.byref(c), -1, ctypes.byref(h)) == 0
    lib.hfg_destroy(h)
    c.resblock_type = 2
    assert lib.hfg_create(ctypes.byref(c), -1, ctypes.byref(h)) == -22
    assert b"resblock_type" in lib.hfg_last_error()
    c.resblock_type = 1
    for bad in (1.5, 1.0, -0.1, float("nan"), float("inf")):
        c.post_slope = bad
        assert lib.hfg_create(ctypes.byref(c), -1, ctypes.byref(h)) == -22, bad
        assert b"post_slope" in lib.hfg_last_error()
    m.resblock_type = 5
    assert lib.hfg_mrf_create(ctypes.byref(m), -1, ctypes.byref(h)) == -22
    assert b"resblock_type" in lib.hfg_last_error()
    with pytest.raises(ValueError):
        pkg.make_config(*args, resblock="3")
    with pytest.raises(ValueError):
        pkg.make_config(*args, final_lrelu_slope=0.0)  # the struct's 0 means 0.1
    # keys of the other block type: refused with a message that names the layout
    h2 = pkg.Handle(pkg.make_config(*args, resblock="2"), -1)
    with pytest.raises(pkg.HfgError) as e:
        h2.set_weight("mrfs.0.resblocks.0.convs1.0.weight", torch.zeros(128, 128, 3))
    assert e.value.code == -22 and "ResBlock2" in str(e.value) and "convs1" in str(e.value)
    h1 = pkg.Handle(pkg.make_config(*args), -1)
    with pytest.raises(pkg.HfgError) as e:
        h1.set_weight("mrfs.0.resblocks.0.convs.0.weight", torch.zeros(128, 128, 3))
    assert e.value.code == -22 and "resblock_type" in str(e.value)
    h1.set_weight("mrfs.0.resblocks.0.convs1.0.weight", torch.zeros(128, 128, 3))
    h2.set_weight("mrfs.0.resblocks.0.convs.0.weight", torch.zeros(128, 128, 3))


def test_type0_handle_byte_counts_unchanged(pkg):
    """The new fields change nothing for a reference-type handle: parameter count,
    workspace bytes (pinned exactly by test_capi_host.py) and, with the release's slope
    set, the same packed layers."""
    args = (80, [8, 8, 2, 2], [16, 16, 4, 4], 512, [3, 7, 11], [[1, 3, 5]] * 3)
    a = pkg.Handle(pkg.make_config(*args, precision="f16x3"), -1)
    b = pkg.Handle(pkg.make_config(*args, precision="f16x3", final_lrelu_slope=0.01), -1)
    lib = pkg.load_library()
    assert lib.hfg_num_params(a.ptr) == lib.hfg_num_params(b.ptr) == 156
    assert a.workspace_bytes(8, 1024) == b.workspace_bytes(8, 1024)
    sd = C.make_state_dict(C.V1, seed=2)
    for hh in (a, b):
        for k, v in sd.items():
            hh.set_weight(k, torch.from_numpy(v))
        hh.commit()
    for mod in ("conv_post", "ups.3", "mrfs.3.resblocks.2.convs2.1"):
        ia, wa, ba = a.packed_layer(mod)
        ib, wb, bb = b.packed_layer(mod)
        assert ia == ib and np.array_equal(wa, wb) and np.array_equal(ba, bb)


def test_release_v3_checkpoint_loads(pkg, S, ckpt):
    """A synthetic release-V3 file: {"generator": sd} with flat resblocks.{N}.convs.{m},
    every conv weight-normed (conv_pre / conv_post included), loads strictly into
    generator_from_release_config(config.json) and folds as torch._weight_norm does."""
    cfg = S.RELEASE_V3
    plain = {k: torch.from_numpy(v) for k, v in S.random_state_dict(cfg, seed=9).items()}
    g = torch.Generator().manual_seed(4)
    rel, want = {}, {}
    for k, v in plain.items():
        parts = k.split(".")
        if parts[0] == "mrfs":  # mrfs.i.resblocks.j.convs.m.* -> resblocks.{3 i + j}.convs.m.*
            flat = ".".join(["resblocks", str(3 * int(parts[1]) + int(parts[3]))] + parts[4:])
        else:
            flat = k
        if flat.endswith(".weight"):
            gshape = (v.shape[0],) + (1,) * (v.dim() - 1)
            wg = v.flatten(1).norm(dim=1).reshape(gshape) * (0.5 + torch.rand(gshape, generator=g))
            rel[flat + "_g"], rel[flat + "_v"] = wg, v
            want[k] = torch._weight_norm(v, wg, 0)
        else:
            rel[flat] = want[k] = v
    assert "resblocks.8.convs.1.weight_g" in rel and "conv_post.weight_v" in rel
    gen = ckpt.generator_from_release_config(V3_JSON)
    assert gen.resblock == "2" and gen.final_lrelu_slope == 0.01
    assert gen._hfg_cfg.resblock_type == 1 and gen._hfg_cfg.post_slope == np.float32(0.01)
    assert gen.n_mels == 80 and gen.num_upsamples == 3
    res = ckpt.load_generator_checkpoint(gen, {"generator": rel}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in gen.state_dict().items():
        assert torch.equal(v, want[k]), k
    # num_mels defaults to 80; a V1 config builds ResBlock (pair) modules with the 0.01 slope
    v1 = ckpt.generator_from_release_config(
        {"resblock": "1", "upsample_rates": [8, 8, 2, 2], "upsample_kernel_sizes": [16, 16, 4, 4],
         "upsample_initial_channel": 512, "resblock_kernel_sizes": [3, 7, 11],
         "resblock_dilation_sizes": [[1, 3, 5]] * 3})
    assert list(v1.state_dict()) == [k for k, _, _ in C.param_specs(C.V1)]
    assert v1._hfg_cfg.resblock_type == 0 and v1._hfg_cfg.post_slope == np.float32(0.01)
    # a V3 file into a default (pair) Generator: no module has those keys
    with pytest.raises(RuntimeError):
        ckpt.load_generator_checkpoint(pkg.HiFiGANGenerator(**C.V2STAR.kwargs()),
                                       {"generator": rel}, strict=True)


def test_synth_release_preset(S):
    cfg = S.RELEASE_V3
    assert cfg.kwargs()["resblock"] == "2" and cfg.kwargs()["final_lrelu_slope"] == 0.01
    assert cfg.upsample_initial_channel == 256 and cfg.upsample_rates == [8, 8, 4]
    assert set(S.PRESETS) == {"v1", "v2star", "nonexact"}  # the oracle's table, unchanged
    keys = [k for k, _, _ in S.param_specs(cfg)]
    assert len(keys) == 2 * (1 + 3 + 3 * 6 + 1) and "mrfs.1.resblocks.2.convs.1.bias" in keys
    # per frame: 3 passes per ResBlock2 conv instead of 5 per pair
    pair = S.GenConfig(**{k: v for k, v in cfg.kwargs().items()
                          if k not in ("resblock", "final_lrelu_slope")})
    diff = S.layer_streaming_bytes_per_frame(pair) - S.layer_streaming_bytes_per_frame(cfg)
    assert diff == 4 * 2 * 6 * (128 * 8 + 64 * 64 + 32 * 256)


@pytest.mark.parametrize("precision", ["bf16x3", "f16x3"])
def test_resblock2_stream_packing_and_windowing(pkg, S, precision):
    """resblock2_bf16x3's launches of release V3: which blocks are fused, halo / W, the A
    stream [wave_m][conv][g][tap][plane][lane][8] with n_dil convs, and the kernel's
    windowing (first conv exact on the window from the margin columns, then the garbage front
    moves in by each later conv's radius) against the un-windowed block in float64."""
    cfg = S.RELEASE_V3
    sd = S.random_state_dict(cfg, seed=43)
    h = pkg.Handle(pkg.make_config(**cfg.kwargs(), precision=precision), -1)
    for k, v in sd.items():
        h.set_weight(k, torch.from_numpy(v))
    h.commit()
    # stage C = 32, k = 7, d = [3, 12]: the pins of the issue
    info, _, _ = h.packed_resblock(2, 2)
    assert (info["fused"], info["C"], info["KT"], info["n_conv"]) == (1, 32, 7, 2)
    assert info["halo"] == 36 and info["W"] == 440
    # C = 128 has whole-block instances for k = 3 only: k = 5 / 7 run layer by layer
    assert [h.packed_resblock(0, j)[0]["fused"] for j in range(3)] == [1, 0, 0]
    assert [h.packed_resblock(1, j)[0]["fused"] for j in range(3)] == [1, 1, 1]
    lane = np.arange(64)
    for i in range(3):
        for j in range(3):
            info, packed, bias = h.packed_resblock(i, j)
            if not info["fused"]:
                continue
            Cc, KT, n_conv = info["C"], info["KT"], info["n_conv"]
            dils = cfg.resblock_dilation_sizes[j]
            assert Cc == 256 >> (i + 1) and KT == cfg.resblock_kernel_sizes[j]
            assert n_conv == len(dils)
            assert info["halo"] == sum((KT - 1) // 2 * d for d in dils[1:])
            nwin = 256 if Cc == 128 or (Cc == 64 and KT == 3) else 512
            assert info["W"] == (nwin - 2 * info["halo"]) & ~3
            u = packed.view(np.uint16).reshape(Cc // 32, n_conv, Cc // 16, KT, 2, 64, 8)
            Ws = []
            for e in range(n_conv):
                mod = f"mrfs.{i}.resblocks.{j}.convs.{e}"
                ew = h.packed_layer(mod)[0]["ew"]
                val = dec(u[:, :, :, :, 0], precision, ew) + dec(u[:, :, :, :, 1], precision, ew)
                W = sd[mod + ".weight"].astype(np.float64)
                rec = np.zeros_like(W)
                for wm in range(Cc // 32):
                    rows = wm * 32 + (lane & 31)
                    for g in range(Cc // 16):
                        for el in range(8):
                            ci = g * 16 + 4 * (lane >> 5) + (el & 3) + 8 * (el >> 2)
                            rec[rows, ci, :] = val[wm, e, g, :, lane, el]
                assert np.abs(rec - W).max() <= SPLIT_TOL[precision] * np.abs(W).max(), mod
                assert np.array_equal(bias[e * Cc:(e + 1) * Cc], sd[mod + ".bias"])
                Ws.append((rec, sd[mod + ".bias"].astype(np.float64)))
            # each conv emulated from the packed stream: windowed vs direct on one short
            # utterance (len < L, ending inside a window)
            rng = np.random.default_rng(5 + 3 * i + j)
            Wc, halo = info["W"], info["halo"]
            L, ln = 3 * Wc // 2 + 37, 3 * Wc // 2 + 5
            x = rng.standard_normal((Cc, L))
            x[:, ln:] = 0.0

            def block(xx, valid):
                for (w, b), d in zip(Ws, dils):
                    xx = xx + _conv_same(_lrelu(xx) * valid, w, b, d)
                return xx

            direct = block(x[:, :ln], np.ones(ln))
            out = np.zeros((Cc, ln))
            r0 = (KT - 1) // 2 * dils[0]
            for t0 in range(0, ln, Wc):
                ws = t0 - halo
                cols = ws - r0 + np.arange(nwin + 2 * r0)
                ve = ((cols >= 0) & (cols < ln)).astype(np.float64)
                xe = np.where(ve > 0, x[:, np.clip(cols, 0, L - 1)], 0.0)
                # conv 0 reads r0 columns of x past either edge and is kept on the window
                xx, valid = xe[:, r0:r0 + nwin], ve[r0:r0 + nwin]
                xx = xx + _conv_same(_lrelu(xe) * ve, Ws[0][0], Ws[0][1], dils[0])[:, r0:r0 + nwin]
                for (w, b), d in zip(Ws[1:], dils[1:]):  # later convs see the window alone
                    xx = xx + _conv_same(_lrelu(xx) * valid, w, b, d)
                n = min(Wc, ln - t0)
                out[:, t0:t0 + n] = xx[:, halo:halo + n]
            assert np.abs(out - direct).max() < 1e-9, (i, j)


def test_single_dilation_block_has_no_halo(pkg):
    mrf = pkg.MRF(64, [3, 7], [[1], [5]], precision="f16x3", resblock="2")
    h = mrf._hip_new_handle(-1)
    for k, t in mrf._hip_weight_items():
        h.set_weight(k, t)
    h.commit()
    for j, nwin in ((0, 256), (1, 512)):
        info, _, _ = h.packed_resblock(0, j)
        assert info["fused"] == 1 and info["n_conv"] == 1
        assert info["halo"] == 0 and info["W"] == nwin
    # fp32 handles and FUSED_RB = 0 have no whole-block launches
    h = pkg._lib.Handle(pkg._lib.make_mrf_config(64, [3], [[1, 2]], "fp32", resblock="2"), -1,
                        mrf=True)
    assert h.packed_resblock(0, 0)[0]["fused"] == 0


def test_unsupported_layer_shape_refused_at_create(pkg):
    """A ResBlock2 conv whose (k - 1) d is beyond every layer kernel's staging window is
    refused by hfg_create (the message names the layer), as for the pair type."""
    lib = pkg.load_library()
    c = pkg.make_config(80, [8, 8, 4], [16, 16, 8], 256, [3, 5, 7], [[1, 2], [2, 6], [3, 40]],
                        resblock="2")
    h = ctypes.c_void_p()
    assert lib.hfg_create(ctypes.byref(c), -1, ctypes.byref(h)) == -22
    msg = lib.hfg_last_error().decode()
    assert "convs.1" in msg and "dilation" in msg


def test_receptive_field_bounds_the_release_v3_reach(pkg, S):
    """receptive_field_frames() of the V3 generator (a ResBlock2's radius is the sum of its
    convs' paddings) is at least the reach, in frames, of a one-frame impulse through the
    float64 restatement."""
    cfg = S.RELEASE_V3
    gen = pkg.HiFiGANGenerator(**cfg.kwargs())
    sd = S.random_state_dict(cfg, seed=3)
    T, t0, hop = 48, 24, 256
    mel = torch.zeros(1, 80, T, dtype=torch.float64)
    a = release_forward(sd, cfg, mel, torch.float64)
    mel[0, :, t0] = 1.0
    b = release_forward(sd, cfg, mel, torch.float64)
    assert a.shape[-1] == T * hop == gen.output_length(T)
    hit = torch.nonzero((a - b)[0, 0]).flatten()
    reach = int(max(t0 - int(hit.min()) // hop, int(hit.max()) // hop - t0))
    rf = gen.receptive_field_frames()
    assert 0 < reach <= rf < T - t0, (reach, rf)
    # the hand sum: conv_pre 3; per stage the upsampler's 2 taps per phase at the input rate,
    # then the widest block (k = 7, d = [3, 12]: 9 + 36) at the output rate; conv_post 3
    want = 3 + 2 + 45 / 8 + 2 / 8 + 45 / 64 + 2 / 64 + 45 / 256 + 3 / 256
    assert rf == int(want) + 1
