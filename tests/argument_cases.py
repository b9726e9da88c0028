"""Cases, inputs, references and guarded buffers of the Generator's argument-edge tests
(tests/test_arguments_host.py on the CPU, tests/test_gpu_arguments.py on the GPU): lengths
outside [1, T], guard bands around every caller-owned buffer, the batch limit, and a batch whose
activation buffers pass 4 GiB.  Plain helpers, not a conftest.

The references are the float64 restatement ``oracle/hifigan_np64.py`` (small items, computed
once per session and shared, never modified) and the torch oracle on windows of long items, at
the project's wav bar of 1e-4.  Everything else is "bitwise the item's solo run".

The mutants at the end restate, in numpy only, three ways the library could go wrong (lengths
clamped into [1, T], an item base reduced modulo 2^32 bytes, a four-wide tail store on a row
whose length is not a multiple of four): the host suite shows that each check of the GPU suite
fails on its mutant.  The project's own code is never made wrong.
"""
import functools

import numpy as np
import torch

from oracle import config as C, prng, hifigan_np64 as N

ATOL = 1e-4   # the project's wav bar
PRECISIONS = ("fp32", "f16x3", "bf16x3", "bf16w")
REF_PRECISIONS = ("fp32", "f16x3", "bf16x3")   # bf16w computes another model (bf16 weights)

# ----------------------------------------------------------------------------------------
# configurations
# ----------------------------------------------------------------------------------------
# "tail": the width suite's W200R (odd rates 3 x 5, stage widths 100 and 50): out_len = 15 T,
# so the wav rows are no multiple of 4 long at odd T
TAIL = C.GenConfig(upsample_rates=[3, 5], upsample_kernel_sizes=[7, 11],
                   upsample_initial_channel=200, resblock_kernel_sizes=[3, 7, 11],
                   resblock_dilation_sizes=[[1, 3], [1, 5], [2, 4]])


def _tiny(c0):
    return C.GenConfig(upsample_rates=[2, 2], upsample_kernel_sizes=[4, 4],
                       upsample_initial_channel=c0, resblock_kernel_sizes=[3, 5],
                       resblock_dilation_sizes=[[1, 3], [1, 3]])


CONFIGS = {
    "v1": C.V1, "v2star": C.V2STAR, "nonexact": C.NONEXACT, "tail": TAIL,
    # the batch-limit cases: stages of 16 and 8 channels (one thin launch per MRF), and of 64
    # and 32 (whole-ResBlock launches and layer convs)
    "tiny32": _tiny(32), "tiny128": _tiny(128),
}
WILD_CONFIGS = ("v1", "v2star", "nonexact", "tail")
SEED = 211


@functools.lru_cache(maxsize=None)
def state(name):
    """Default-init-bounded PRNG weights of a configuration (shared: never modified)."""
    sd = C.make_state_dict(CONFIGS[name], seed=SEED)
    for v in sd.values():
        v.setflags(write=False)
    return sd


def torch_state(name):
    """The torch oracle's state of a configuration (its own copies of the shared weights)."""
    from oracle import hifigan_torch as H
    return H.to_torch_state({k: np.array(v) for k, v in state(name).items()})


def make_generator(pkg, name, precision, dev, knobs=None):
    """The module of a configuration on `dev`, its handle created under the schedule overrides
    `knobs` (read when the handle is created); only the knobs set here are cleared."""
    knobs = knobs or {}
    try:
        for k, v in knobs.items():
            pkg.schedule_override(k, int(v))
        gen = pkg.HiFiGANGenerator(**CONFIGS[name].kwargs(), precision=precision).eval()
        gen.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state(name).items()})
        gen = gen.to(dev)
        gen.hip_handle(dev)
    finally:
        for k in knobs:
            pkg.schedule_clear(k)
    return gen


def host_handle(pkg, name, precision):
    """A host-only handle of the configuration (sizes, layout and plan need no device)."""
    return pkg.Handle(pkg.make_config(**CONFIGS[name].kwargs(), precision=precision), -1)


# ----------------------------------------------------------------------------------------
# wild and empty lengths
# ----------------------------------------------------------------------------------------
WILD_T = 37
WILD = [10 ** 9, -4, 0, WILD_T, 1, WILD_T + 1, 36, -2 ** 31]
WILD_REF_ITEMS = (0, 4, 6)   # a full item, one frame, T - 1 frames


def clamped(lens, T):
    """What the library makes of a length vector: every entry clamped into [0, T]."""
    return [min(max(n, 0), T) for n in lens]


def nan_padded(mel, lens):
    """A copy of mel [B, n_mels, T] with NaN in every frame at or past the item's length (an
    item of length 0 is all NaN): padding that a kernel masking by multiplication lets through."""
    out = np.array(mel, dtype=np.float32)
    for b, n in enumerate(lens):
        out[b, :, n:] = np.nan
    return out


@functools.lru_cache(maxsize=None)
def wild_mel(name):
    """The wild case's mel [8, n_mels, WILD_T], NaN past every clamped length (shared)."""
    m = nan_padded(prng.mel_input(SEED + 1, (len(WILD), CONFIGS[name].n_mels, WILD_T)),
                   clamped(WILD, WILD_T))
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def wild_ref(name, b, n=None):
    """float64 reference wav [L] of item b of the wild case on its first n frames (default: its
    clamped length).  Shared, read-only."""
    n = clamped(WILD, WILD_T)[b] if n is None else n
    w = N.generator_forward(state(name), CONFIGS[name], np.array(wild_mel(name)[b:b + 1, :, :n]))
    w = w[0, 0]
    w.setflags(write=False)
    return w


def ragged_reference(name, mel, lens, lo=0):
    """float64 restatement of a ragged forward on wild lengths: item b is the reference on its
    first clamp(lens[b]) frames, zero past its own output, an empty item a zero row.
    ``lo`` is the lower clamp: 0 restates the library, 1 is the mutant that lets no item be
    empty."""
    B, _, T = mel.shape
    out = np.zeros((B, C.out_len(CONFIGS[name], T)))
    for b, n in enumerate(lens):
        n = min(max(n, lo), T)
        if n > 0:
            w = N.generator_forward(state(name), CONFIGS[name], mel[b:b + 1, :, :n])[0, 0]
            out[b, :w.shape[0]] = w
    return out


# ----------------------------------------------------------------------------------------
# the batch limit
# ----------------------------------------------------------------------------------------
MAX_BATCH = 65535
LIMIT_ITEMS = (0, 1, 32767, 32768, 65534)   # both ends and both sides of the two-stream cut


@functools.lru_cache(maxsize=None)
def limit_mel(name):
    """[MAX_BATCH, n_mels, 1]: one frame per item, every item different (shared)."""
    m = prng.mel_input(SEED + 2, (MAX_BATCH, CONFIGS[name].n_mels, 1))
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def limit_ref(name):
    """{item: float64 reference wav [L]} of LIMIT_ITEMS of limit_mel(name)."""
    m = limit_mel(name)
    return {b: N.generator_forward(state(name), CONFIGS[name], np.array(m[b:b + 1]))[0, 0]
            for b in LIMIT_ITEMS}


def planted_zeros(B, n=10, seed=SEED + 3):
    """n distinct positions in [0, B) for empty items: 0, B - 1 and seeded ones between."""
    u = prng.uniform01(seed, "empty items", 4 * n)
    pos = [0, B - 1]
    for v in u:
        p = 1 + int(v * (B - 2))
        if p not in pos and len(pos) < n:
            pos.append(p)
    assert len(pos) == n
    return sorted(pos)


# ----------------------------------------------------------------------------------------
# guarded buffers
# ----------------------------------------------------------------------------------------
BAND = 4096
PATTERN = 0xA5
ALIGN = 256


class Banded:
    """``nbytes`` of device memory between two BAND-byte bands of PATTERN."""

    def __init__(self, nbytes, dev):
        self.nbytes = nbytes
        self.buf = torch.full((nbytes + 2 * BAND,), PATTERN, dtype=torch.uint8, device=dev)
        self.ptr = self.buf.data_ptr() + BAND

    def assert_bands_untouched(self):
        torch.cuda.synchronize()
        assert bool((self.buf[:BAND] == PATTERN).all()), "write below the workspace"
        assert bool((self.buf[BAND + self.nbytes:] == PATTERN).all()), "write past the workspace"


class Arena:
    """A tensor ``.t`` of the asked shape (float32 or int32) inside a larger allocation: at least
    BAND bytes of ``fill`` on both sides, the payload ALIGN-byte aligned and filled too.  A kernel
    that stores past a row of the last item, or before the first, changes a band; one that uses
    a value read from a NaN band shows it in its output."""

    def __init__(self, shape, fill, dev, dtype=torch.float32):
        n = int(np.prod(shape))
        words = n + (2 * BAND + ALIGN) // 4
        self.buf = torch.full((words,), fill, dtype=dtype, device=dev)
        self.lo = (BAND + (-(self.buf.data_ptr() + BAND)) % ALIGN) // 4
        self.hi = self.lo + n
        self.t = self.buf[self.lo:self.hi].view(shape)
        assert self.t.data_ptr() % ALIGN == 0 and self.lo * 4 >= BAND
        assert (words - self.hi) * 4 >= BAND
        # compared as bits: NaN != NaN
        self.bits = torch.full((1,), fill, dtype=dtype).view(torch.int32).item()

    def put(self, value):
        self.t.copy_(value)
        return self

    def assert_bands_untouched(self, what):
        torch.cuda.synchronize()
        bits = self.buf.view(torch.int32)
        assert bool((bits[:self.lo] == self.bits).all()), f"write below {what}"
        assert bool((bits[self.hi:] == self.bits).all()), f"write past {what}"


# ----------------------------------------------------------------------------------------
# a batch past 4 GiB per buffer
# ----------------------------------------------------------------------------------------
HUGE_B, HUGE_T = 5, 32768   # V1 stages 1-3: 8192 T floats per item = 2^30 bytes


# ----------------------------------------------------------------------------------------
# mutants of the restatement (sensitivity; tests/test_arguments_host.py)
# ----------------------------------------------------------------------------------------
def store_items(items, modulus_bytes=None):
    """The kernels' addressing of a [B][n] fp32 activation buffer, restated: item b is stored
    at, and read back from, byte base b * 4 n, offsets inside the item added to it.
    ``modulus_bytes``: the mutant that reduces the base modulo that many bytes (the dropped
    (int64_t) reduces it modulo 2^32; here scaled down to a small buffer).  Items are stored in
    batch order, then all read back: what a consumer launch sees."""
    items = np.asarray(items, dtype=np.float32)
    B, n = items.shape
    buf = np.zeros(B * n, dtype=np.float32)

    def base(b):
        byte = b * 4 * n
        return (byte % modulus_bytes if modulus_bytes else byte) // 4

    for b in range(B):
        buf[base(b):base(b) + n] = items[b]
    return np.stack([buf[base(b):base(b) + n] for b in range(B)])


def store_rows(rows, band, fill, quad_tail=False):
    """An epilogue's stores of rows [R][L] into a buffer followed by a band of ``fill``: whole
    groups of four as one store, the last L % 4 samples one by one.  ``quad_tail``: the mutant
    that stores the tail group four wide too (lanes past the row's end carry zeros).  The rows
    are written last to first, as blocks of one launch may retire.  Returns (rows read back,
    band)."""
    rows = np.asarray(rows, dtype=np.float32)
    R, L = rows.shape
    buf = np.full(R * L + band, fill, dtype=np.float32)
    for r in reversed(range(R)):
        for i in range(0, L, 4):
            w = 4 if (i + 4 <= L or quad_tail) else L - i
            v = np.zeros(w, dtype=np.float32)
            v[:min(w, L - i)] = rows[r, i:i + w]
            buf[r * L + i:r * L + i + w] = v
    return buf[:R * L].reshape(R, L), buf[R * L:]
