"""Print the A/B runs of profiles/ab_run.sh: value, ms/step, per-kernel ms, the wav checksums of
every precision and (DUMP=1 runs) the sha256 of each dumped wav.npy.
usage: python profiles/ab_show.py TAG"""
import glob
import hashlib
import json
import os
import re
import sys

tag = sys.argv[1] if len(sys.argv) > 1 else "ab"
out = os.environ.get("OUT_DIR", "profiles/out")
files = sorted(glob.glob(f"{out}/{tag}_old*.json") + glob.glob(f"{out}/{tag}_new*.json"),
               key=lambda f: (int(re.search(r"(\d+)\.json$", f).group(1)), "new" in os.path.basename(f)))
for f in files:
    d = json.loads(open(f).read().strip().splitlines()[-1])
    ks = {k.split("(")[0][:34]: round(v["ms_per_step"], 4) for k, v in d.get("kernels", {}).items()
          if v["ms_per_step"] > 0.1}
    sums = {"main": d.get("wav_checksum32")}
    sums.update({p: a.get("wav_checksum32") for p, a in (d.get("alt") or {}).items()
                 if isinstance(a, dict)})
    wav = f[:-5] + "/wav.npy"
    sha = hashlib.sha256(open(wav, "rb").read()).hexdigest()[:16] if os.path.exists(wav) else None
    print(os.path.basename(f)[len(tag) + 1:-5], "value", round(d.get("value", 0) / 1e6, 2),
          "ms", round(d["ms_per_step"], 4), "sums", sums, "wav.npy", sha, ks)
