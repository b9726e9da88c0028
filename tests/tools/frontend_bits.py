#!/usr/bin/env python3
"""One sha256 per audio front-end output, for a bitwise A/B of two builds of the library
(needs the GPU).

    python tests/tools/frontend_bits.py LIBRARY OUT.json

Runs mel.MelSpectrogram, mel.ReleaseMelSpectrogram and mel.Resample (fixed-length and ragged)
through the package with LIBRARY loaded, over the shapes of tests/mel_cases.py, the release-mel
cases of tests/test_gpu_release_mel.py and the batches of tests/ragged_resample_cases.py, plus
the README shape [8, 262144], and writes {case: sha256 of the raw output bytes}.  Run it once
per library, each in a fresh process (HFG_ALLOW_OLD_LIB=1 admits a library that is not this
tree's build), and compare the two files: every hash must be equal."""
import hashlib
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main() -> int:
    lib_path, out_path = sys.argv[1:3]
    import __graft_entry__ as ge
    pkg = ge.load_package()
    pkg.load_library(os.path.abspath(lib_path))      # cached: every later call uses this one
    M = importlib.import_module(ge.PKG_NAME + ".mel")
    import mel_cases as MC
    import ragged_resample_cases as RC
    from release_mel_oracle import signals
    dev = torch.device("cuda:0")
    out = {}

    def put(case, *tensors):
        torch.cuda.synchronize()
        h = hashlib.sha256()
        for t in tensors:
            h.update(t.cpu().contiguous().numpy().tobytes())
        out[case] = h.hexdigest()

    for cfg in MC.FFT_CONFIGS + MC.DFT_CONFIGS + [MC.DFT_FORCED]:
        if cfg is MC.DFT_FORCED:
            pkg.schedule_override("MEL_DFT", 1)
        ext = M.MelSpectrogram(**MC.class_kwargs(cfg), device=dev)
        pkg.schedule_clear("MEL_DFT")
        for n in MC.lengths(cfg):
            put(f"mel/{cfg['name']}/{n}", ext(MC.mel_batch(n, cfg["sample_rate"]).to(dev)))

    front = M.ReleaseMelSpectrogram(device=dev)
    for n in (385, 513, 4173, 8269):
        put(f"relmel/default/{n}", front(signals(n).to(dev)))
    for n_fft, hop, win in ((512, 128, 512), (2048, 512, 2048), (256, 64, 256), (1024, 256, 800)):
        ext = M.ReleaseMelSpectrogram(n_fft=n_fft, hop_size=hop, win_size=win, device=dev)
        put(f"relmel/{n_fft}_{hop}_{win}/7000", ext(signals(7000).to(dev)))
    s = signals(8269)
    put("relmel/ragged", *front(torch.stack([s[0], s[1], 0.5 * (s[0] + s[1])]).to(dev),
                                [8269, 3000, 385]))

    for (orig, new) in list(MC.RESAMPLE_PAIRS) + [RC.IDENTITY]:
        rs = M.Resample(orig, new, device=dev)
        if (orig, new) != RC.IDENTITY:
            for n in MC.resample_lengths(orig, new):
                put(f"resample/{orig}-{new}/{n}", rs(torch.tensor(MC.resample_rows(n, 7)).to(dev)))
        x32, x16 = torch.tensor(RC.signal(orig, new)), torch.tensor(RC.signal_s16(orig, new))
        for i, lens in enumerate(RC.batches(orig, new)):
            for C in RC.CHANNELS:
                for x in (x32, x16):
                    put(f"ragged/{orig}-{new}/{i}/C{C}/{x.dtype}",
                        *rs.ragged(x[:, :C].contiguous().to(dev), lens))

    g = torch.Generator().manual_seed(0)
    wav = torch.randn(8, 262144, generator=g).clamp(-1, 1).to(dev)
    lens = [262144 - 997 * b for b in range(8)]
    put("readme/mel", M.MelSpectrogram(device=dev)(wav))
    put("readme/relmel", front(wav))
    put("readme/relmel_ragged", *front(wav, lens))
    rs = M.Resample(48000, 22050, device=dev)
    put("readme/resample", rs(wav))
    put("readme/resample_ragged", *rs.ragged(wav, lens))
    stereo = (wav.view(4, 2, -1) * 20000).round().to(torch.int16)
    put("readme/resample_ragged_stereo_s16", *rs.ragged(stereo, lens[:4]))

    with open(out_path, "w") as f:
        json.dump({"library": pkg.load_library().hfg_version().decode(), "sha256": out}, f,
                  indent=1, sort_keys=True)
    print(f"frontend_bits: {len(out)} cases -> {out_path}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
