"""The argument-edge suite's CPU half (tests/argument_cases.py, tests/test_gpu_arguments.py):

* the batch limit on host-only handles: the public sizes accept B = 65535 and return 0 for
  65536, the entries that take a B refuse it with HFG_EINVAL;
* the workspace layout of the batch whose buffers pass 4 GiB (V1, 5 x 32768 frames);
* the reference-side conditions that make the wild-length checks mean something: the one-frame
  and the T - 1 item are not silence, and a length off by one frame moves the full item's last
  hop by more than the wav bar;
* sensitivity: each check of the GPU suite fails on a mutant of the numpy restatement (lengths
  clamped into [1, T]; an item base reduced modulo the buffer's "4 GiB"; a four-wide tail store
  on an L % 4 == 2 row).  The project's code is never made wrong.
"""
import numpy as np
import pytest
import torch

import argument_cases as A
from oracle import config as C


# ---- the batch axis ---------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
@pytest.mark.parametrize("name", ["v1", "tiny32", "tiny128"])
def test_workspace_sizes_stop_at_the_batch_limit(pkg, name, precision):
    h = A.host_handle(pkg, name, precision)
    assert h.workspace_bytes(A.MAX_BATCH, 1) > 0
    assert h.workspace_bytes(A.MAX_BATCH + 1, 1) == 0
    assert h.workspace_layout(A.MAX_BATCH, 1)["total"] == h.workspace_bytes(A.MAX_BATCH, 1)
    with pytest.raises(pkg.HfgError, match=r"B must be in \[1, 65535\]") as e:
        h.workspace_layout(A.MAX_BATCH + 1, 1)
    assert e.value.code == -22


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
@pytest.mark.parametrize("channels", [64, 32])
def test_mrf_workspace_sizes_stop_at_the_batch_limit(pkg, channels, precision):
    cfg = pkg._lib.make_mrf_config(channels, [3, 7, 11], [[1, 3, 5]] * 3, precision)
    h = pkg.Handle(cfg, -1, mrf=True)
    assert h.mrf_workspace_bytes(A.MAX_BATCH, 1) > 0
    assert h.mrf_workspace_bytes(A.MAX_BATCH + 1, 1) == 0


def test_reserve_refuses_a_batch_over_the_limit(pkg):
    """hfg_reserve on a host-only handle refuses for the handle; on any handle B = 65536 is
    EINVAL too (the GPU suite checks the message on a device handle)."""
    h = A.host_handle(pkg, "tiny32", "fp32")
    assert h.lib.hfg_reserve(h.ptr, A.MAX_BATCH + 1, 1) == -22


def test_module_refuses_a_batch_over_the_limit_before_it_allocates(pkg):
    """HiFiGANGenerator.forward / MRF.forward / ResBlock.forward check B before they look at
    the device or allocate: a meta tensor of 65536 items costs no memory and never reaches the
    library."""
    gen = pkg.HiFiGANGenerator(**A.CONFIGS["tiny32"].kwargs(), precision="fp32").eval()
    mel = torch.empty(A.MAX_BATCH + 1, 80, 1, device="meta")
    with pytest.raises(RuntimeError, match=r"B must be in \[1, 65535\]"):
        gen(mel)
    with pytest.raises(RuntimeError, match=r"B must be in \[1, 65535\]"):
        gen.forward_with_stages(mel)
    x = torch.empty(A.MAX_BATCH + 1, 16, 4, device="meta")
    with pytest.raises(RuntimeError, match=r"B must be in \[1, 65535\]"):
        gen.mrfs[0](x)
    with pytest.raises(RuntimeError, match=r"B must be in \[1, 65535\]"):
        gen.mrfs[0].resblocks[0](x)


def test_empty_item_has_no_samples(pkg):
    """output_length(0) == 0 in every configuration, as the device's stage-length table has it
    (a non-exact stage would otherwise make k - u samples of nothing)."""
    for name in A.WILD_CONFIGS:
        gen = pkg.HiFiGANGenerator(**A.CONFIGS[name].kwargs(), precision="fp32")
        assert gen.output_length(0) == 0 and gen.output_length(-3) == 0
        for t in (1, 2, A.WILD_T):
            assert gen.output_length(t) == C.out_len(A.CONFIGS[name], t)


@pytest.mark.parametrize("name,streams,parts", [("tiny32", 1, [65535]), ("tiny32", 2, [32768, 32767]),
                                                ("tiny128", 1, [65535]), ("tiny128", 2, [32768, 32767])])
def test_batch_limit_layout_parts(pkg, name, streams, parts):
    h = A.host_handle(pkg, name, "f16x3")
    h.set_streams(streams)
    assert [p["B"] for p in h.workspace_layout(A.MAX_BATCH, 1)["parts"]] == parts


def test_batch_limit_paths(pkg):
    """tiny32 runs both MRFs as thin launches, tiny128 none: the two cases of the GPU suite put
    B = 65535 on different kernels' grids."""
    for name, thin in (("tiny32", [1, 1]), ("tiny128", [0, 0])):
        for precision in ("fp32", "f16x3"):
            h = A.host_handle(pkg, name, precision)
            for k, v in A.state(name).items():
                h.set_weight(k, torch.from_numpy(np.array(v)))
            assert [int(bool(s["thin"])) for s in h.plan()["stages"]] == thin, (name, precision)


# ---- a batch past 4 GiB per buffer ----------------------------------------------------------
@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
@pytest.mark.parametrize("streams,parts", [(1, [5]), (2, [3, 2])])
def test_huge_batch_layout(pkg, precision, streams, parts):
    h = A.host_handle(pkg, "v1", precision)
    h.set_streams(streams)
    lay = h.workspace_layout(A.HUGE_B, A.HUGE_T)
    assert [p["B"] for p in lay["parts"]] == parts
    regions = [r for p in lay["parts"] for r in p["regions"] if r["bytes"]]
    end = 0
    for r in regions:
        assert r["off"] % 256 == 0, r
        assert r["off"] >= end, (r, "overlaps the region before it")
        end = r["off"] + r["bytes"]
    assert end == lay["total"] == h.workspace_bytes(A.HUGE_B, A.HUGE_T)
    assert sum(r["off"] >= 2 ** 32 for r in regions) >= 3
    # stages 1-3 hold 2^30 bytes per item: item 2 of a buffer starts 2^31 bytes in, item 4 2^32
    item = 4 * max(c * l for c, l in zip((256, 128, 64, 32),
                                         (8 * A.HUGE_T, 64 * A.HUGE_T, 128 * A.HUGE_T, 256 * A.HUGE_T)))
    assert item == 2 ** 30
    for p in lay["parts"]:
        for r in p["regions"][:4]:
            assert r["bytes"] >= p["B"] * item
    if streams == 2:
        assert all(r["off"] >= 12 * 2 ** 30 for r in lay["parts"][1]["regions"])


# ---- reference-side conditions ----------------------------------------------------------
@pytest.mark.parametrize("name", A.WILD_CONFIGS)
def test_wild_case_references_can_tell(name):
    cfg = A.CONFIGS[name]
    T = A.WILD_T
    assert A.clamped(A.WILD, T) == [T, 0, 0, T, 1, T, T - 1, 0]
    m = A.wild_mel(name)
    for b, n in enumerate(A.clamped(A.WILD, T)):
        assert np.isfinite(m[b, :, :n]).all() and np.isnan(m[b, :, n:]).all()
    for b in (4, 6):
        assert np.abs(A.wild_ref(name, b)).max() > 1e-3, b
    full, crop = A.wild_ref(name, 0), A.wild_ref(name, 0, T - 1)
    assert full.shape[0] == C.out_len(cfg, T) and crop.shape[0] == C.out_len(cfg, T - 1)
    hop = C.out_len(cfg, T) - C.out_len(cfg, T - 1)
    padded = np.zeros_like(full)
    padded[:crop.shape[0]] = crop
    # a clamp to T - 1 loses the last hop ...
    assert np.abs(full - padded)[-hop:].max() > 1e-4
    # ... and moves the samples before it: the last frame reaches back over the cut
    assert np.abs(full - padded)[-2 * hop:-hop].max() > 1e-4


# ---- sensitivity, on the restatement only -----------------------------------------------
def test_mutant_lengths_clamped_to_one_make_the_empty_row_nonzero():
    name = "v2star"
    T = A.WILD_T
    mel = np.array(A.wild_mel(name))
    good = A.ragged_reference(name, mel, A.WILD, lo=0)
    empty = [b for b, n in enumerate(A.clamped(A.WILD, T)) if n == 0]
    assert empty == [1, 2, 7]
    assert np.isfinite(good).all() and not good[empty].any()
    for b in A.WILD_REF_ITEMS:
        w = A.wild_ref(name, b)
        assert np.array_equal(good[b, :w.shape[0]], w) and not good[b, w.shape[0]:].any()
    bad = A.ragged_reference(name, mel, A.WILD, lo=1)
    # an empty item run on its first frame: NaN here, and on any finite mel a nonzero row
    assert not np.isfinite(bad[empty]).all()
    finite = np.nan_to_num(mel, nan=0.25)
    bad = A.ragged_reference(name, finite, A.WILD, lo=1)
    for b in empty:
        assert np.abs(bad[b]).max() > 1e-3, b
    assert np.array_equal(bad[[0, 3, 4, 5, 6]], good[[0, 3, 4, 5, 6]])


def test_mutant_item_base_modulo_wraps_item_four_onto_item_zero():
    """The same index arithmetic as a [5][n] fp32 buffer of 2^30-byte items, scaled down: with
    the base reduced modulo 4 items' bytes, item 4 is stored over item 0 and read back for
    both, which "item 4 != item 0" and "item 0 is its solo run" notice."""
    n = 24
    items = np.arange(5 * n, dtype=np.float32).reshape(5, n) + 1.0
    good = A.store_items(items)
    assert np.array_equal(good, items)
    assert not np.array_equal(good[4], good[0])
    bad = A.store_items(items, modulus_bytes=4 * 4 * n)
    assert np.array_equal(bad[4], bad[0])          # the condition of the GPU test fails
    assert not np.array_equal(bad[0], items[0])    # and so does item 0 against its solo run
    assert np.array_equal(bad[1:], items[1:])
    # a signed wrap at half the range moves item 2 instead: caught by its solo run
    bad = A.store_items(items, modulus_bytes=2 * 4 * n)
    assert not np.array_equal(bad[0], items[0]) and np.array_equal(bad[2], bad[0])


def test_mutant_quad_tail_store_reaches_the_next_row_and_the_band():
    R, L, band = 3, 10, 16   # L % 4 == 2
    rows = np.arange(R * L, dtype=np.float32).reshape(R, L) + 1.0
    got, after = A.store_rows(rows, band, fill=-7.5)
    assert np.array_equal(got, rows) and (after == -7.5).all()
    got, after = A.store_rows(rows, band, fill=-7.5, quad_tail=True)
    assert np.array_equal(got[0], rows[0])
    for r in (1, 2):   # the row above stored two lanes past its end
        assert not np.array_equal(got[r], rows[r]) and not got[r, :2].any()
    assert not (after == -7.5).all() and (after[2:] == -7.5).all()
    # rows of a multiple of four are whole groups: the wide store is the right one there
    rows = rows[:, :8].copy()
    got, after = A.store_rows(rows, band, fill=-7.5, quad_tail=True)
    assert np.array_equal(got, rows) and (after == -7.5).all()
