"""The launch schedule stays inside the workspace the public sizes promise (csrc/handle.h
``WsLayout``): the C-ABI forward run on a workspace of exactly ``hfg_workspace_bytes``
(``hfg_mrf_workspace_bytes``) bytes that sits between two 4096-byte bands of a byte pattern
leaves both bands untouched, and its output is bitwise the module's own forward.  A correct
layout never reaches the bands: nothing here provokes an out-of-bounds access.

Cases, each in f16x3 and fp32: V2* 3 x 1366 frames with ragged lengths (two unequal halves,
B * T just over the split threshold), V1 1 x 16 (one part with concurrent ResBlocks and
their triples), ``hfg_forward_taps`` on the first shape (the whole batch as one part inside
the split-sized workspace), and an MRF handle (C = 64, 2 x 259) by default and layer by
layer (FUSED_RB = 0, the R / Tb path).
"""
import pytest
import torch

from argument_cases import Banded
from oracle import config as C, prng

pytestmark = pytest.mark.gpu

PRECISIONS = ["f16x3", "fp32"]
RAGGED = (3, 1366, [1366, 901, 37])   # B, T, valid frames per item


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def _gen(pkg, cfg, precision, dev, seed):
    gen = pkg.HiFiGANGenerator(**cfg.kwargs(), precision=precision).eval()
    gen.load_state_dict({k: torch.from_numpy(v) for k, v in C.make_state_dict(cfg, seed).items()})
    return gen.to(dev)


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


@pytest.fixture(scope="module")
def ragged_mel():
    B, T, _ = RAGGED
    return torch.from_numpy(prng.mel_input(41, (B, C.V2STAR.n_mels, T)))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_split_ragged_forward_stays_inside(pkg, ragged_mel, precision):
    dev = _dev()
    B, T, lengths = RAGGED
    gen = _gen(pkg, C.V2STAR, precision, dev, seed=41)
    mel = ragged_mel.to(dev)
    lens = torch.tensor(lengths, dtype=torch.int32, device=dev)
    with torch.no_grad():
        want = gen(mel, lengths=lens)
    h = gen.hip_handle(dev)
    assert len(h.workspace_layout(B, T)["parts"]) == 2
    ws = Banded(h.workspace_bytes(B, T), dev)
    wav = torch.empty_like(want)
    h.forward_ex(mel.data_ptr(), B, T, wav.data_ptr(), h.out_len(T), ws.ptr, ws.nbytes,
                 _stream(dev), lengths_ptr=lens.data_ptr())
    ws.assert_bands_untouched()
    assert torch.equal(wav, want)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_concurrent_resblock_forward_stays_inside(pkg, precision):
    dev = _dev()
    B, T = 1, 16
    gen = _gen(pkg, C.V1, precision, dev, seed=42)
    mel = torch.from_numpy(prng.mel_input(42, (B, C.V1.n_mels, T))).to(dev)
    with torch.no_grad():
        want = gen(mel)
    h = gen.hip_handle(dev)
    part, = h.workspace_layout(B, T)["parts"]
    assert any(r["name"] == "rb0.out" for r in part["regions"])
    ws = Banded(h.workspace_bytes(B, T), dev)
    wav = torch.empty_like(want)
    h.forward_ws(mel.data_ptr(), B, T, wav.data_ptr(), h.out_len(T), ws.ptr, ws.nbytes,
                 _stream(dev))
    ws.assert_bands_untouched()
    assert torch.equal(wav, want)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_taps_forward_stays_inside_the_split_workspace(pkg, ragged_mel, precision):
    dev = _dev()
    B, T, _ = RAGGED
    gen = _gen(pkg, C.V2STAR, precision, dev, seed=41)
    mel = ragged_mel.to(dev)
    with torch.no_grad():
        want = gen(mel)
    h = gen.hip_handle(dev)
    assert len(h.workspace_layout(B, T, taps=True)["parts"]) == 1
    ws = Banded(h.workspace_bytes(B, T), dev)
    wav = torch.empty_like(want)
    n_taps = 1 + 2 * len(C.V2STAR.upsample_rates)
    h.forward_taps(mel.data_ptr(), B, T, wav.data_ptr(), h.out_len(T), ws.ptr, ws.nbytes,
                   [0] * n_taps, _stream(dev))
    ws.assert_bands_untouched()
    assert torch.equal(wav, want)


@pytest.mark.parametrize("fused_rb", [1, 0], ids=["default", "FUSED_RB=0"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_mrf_forward_stays_inside(pkg, sched, precision, fused_rb):
    dev = _dev()
    B, ch, L = 2, 64, 259
    if not fused_rb:
        sched("FUSED_RB", 0)
    torch.manual_seed(43)
    mrf = pkg.MRF(ch, precision=precision).eval().to(dev)
    x = (torch.randn(B, ch, L) * 0.5).to(dev)
    with torch.no_grad():
        want = mrf(x)
    h = mrf._handle_for(dev)
    ws = Banded(h.mrf_workspace_bytes(B, L), dev)
    y = torch.empty_like(want)
    h.mrf_forward(x.data_ptr(), B, L, y.data_ptr(), ws.ptr, ws.nbytes, _stream(dev))
    ws.assert_bands_untouched()
    assert torch.equal(y, want)
