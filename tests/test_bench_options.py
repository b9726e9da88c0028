"""bench.py's run modes: a plain run measures the headline pass only, ``--full`` switches
the other measurements on, ``--dump-outputs DIR`` writes the wav of the last timed step."""
import importlib
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _parse(bench, monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_switches_every_extra_off(bench, monkeypatch):
    a = _parse(bench, monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert not a.full and a.steps == 7 and a.warmup == 2 and a.dump_outputs is None
    assert a.also == []
    assert a.no_profile and a.no_pmc and a.no_extra and a.no_cpu_baseline
    # the flags of a --full run's own options are accepted (and change nothing) without it
    a = _parse(bench, monkeypatch, "--no-extra", "--no-cpu-baseline", "--no-pmc", "--also")
    assert a.also == [] and a.no_profile


def test_full_run_keeps_the_extras_and_their_switches(bench, monkeypatch):
    a = _parse(bench, monkeypatch, "--full")
    assert a.full and a.also == ["bf16x3", "fp32", "bf16w"]
    assert not (a.no_profile or a.no_pmc or a.no_extra or a.no_cpu_baseline)
    a = _parse(bench, monkeypatch, "--full", "--also", "fp32", "--no-pmc")
    assert a.also == ["fp32"] and a.no_pmc and not a.no_extra
    assert _parse(bench, monkeypatch, "--full", "--also").also == []


def test_other_precisions_need_full(bench, monkeypatch, capsys):
    with pytest.raises(SystemExit) as e:
        _parse(bench, monkeypatch, "--also", "fp32")
    assert e.value.code == 2 and "--full" in capsys.readouterr().err


def test_dump_outputs_whole_and_sampled(bench, tmp_path, monkeypatch):
    wav = np.linspace(-1.0, 1.0, 2 * 1 * 4096, dtype=np.float32).reshape(2, 1, 4096)
    bench.dump_outputs(str(tmp_path / "a" / "b"), wav)
    got = np.load(tmp_path / "a" / "b" / "wav.npy")
    assert got.dtype == np.float32 and np.array_equal(got, wav)
    # above the limit: a fixed sample of the elements, the same every time, within the limit
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4 * 1024 + 4 * 1000)
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), wav)
    s1, s2 = np.load(tmp_path / "s1" / "wav.npy"), np.load(tmp_path / "s2" / "wav.npy")
    assert s1.dtype == np.float32 and s1.ndim == 1 and 500 < s1.size <= 1000
    assert np.array_equal(s1, s2)
    assert os.path.getsize(tmp_path / "s1" / "wav.npy") <= bench.DUMP_LIMIT_BYTES
    assert np.all(np.diff(s1) > 0)  # distinct elements of the (increasing) input, in order


@pytest.mark.gpu
def test_plain_run_line_and_dumped_wav(pkg, tmp_path):
    """One plain run at a small shape: the line holds the headline fields and none of the
    --full measurements, and DIR/wav.npy is the wav of bench.py's seeded mel and weights
    (within the suite's 1e-4 parity bar of the CPU oracle)."""
    import torch
    from oracle import config as OC, hifigan_torch
    import __graft_entry__ as ge

    B, T, steps = 3, 33, 2
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
           "--warmup", "1", "--batch", str(B), "--frames", str(T),
           "--dump-outputs", str(tmp_path / "out")]
    r = subprocess.run(["timeout", "-k", "10", "120"] + cmd, cwd=ROOT, capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["steps"] == steps and line["full"] is False
    assert line["unit"] == "audio samples/s" and line["higher_is_better"] is True
    assert line["dtype"] == "f16x3" and line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(B * T * 256 / (line["ms_per_step"] * 1e-3), rel=1e-9)
    for key in ("alt", "roofline", "roofline_step", "kernels", "end_to_end", "extra_configs",
                "cpu_baseline"):
        assert key not in line, key
    assert os.listdir(tmp_path / "out") == ["wav.npy"]
    wav = np.load(tmp_path / "out" / "wav.npy")
    assert wav.dtype == np.float32 and wav.shape == (B, 1, T * 256)

    S = importlib.import_module(ge.PKG_NAME + ".synth")
    cfg = OC.GenConfig(**S.V1.kwargs())
    sd = S.random_state_dict(S.V1, seed=0)
    mel = torch.randn(B, cfg.n_mels, T, generator=torch.Generator().manual_seed(1234))
    with torch.no_grad():
        ref = hifigan_torch.generator_forward(hifigan_torch.to_torch_state(sd), cfg, mel).numpy()
    err = float(np.abs(wav - ref).max())
    print(f"max|dumped wav - oracle| = {err:.3e} (max|ref| {np.abs(ref).max():.3e})")
    assert err < 1e-4
