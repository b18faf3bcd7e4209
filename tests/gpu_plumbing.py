"""Device plumbing of the GPU tests: tensors, stream ids, prefilled buffers, the one factory of contexts.  No tests here; torch
and lyra_amd are imported inside the functions."""
import numpy as np

FILL = 85   # every byte of a prefilled buffer: what a call must not write still holds it afterwards


def _dev():
    import torch
    return torch.device("cuda", 0)


def _t(a, dtype=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype))).to(_dev())


def _ids(B, max_streams, seed):
    return np.random.default_rng(seed).permutation(max_streams)[:B].astype(np.int32)


def _filled(dev, frames, width, dtype):
    """[frames][width] of `dtype`, every byte FILL: a device tensor on `dev`, a numpy array for dev=None"""
    a = np.full((frames, width * np.dtype(dtype).itemsize), FILL, np.uint8).view(dtype)
    if dev is None:
        return a
    import torch
    return torch.from_numpy(a).to(dev)


def _same(got, want, where, names=("pcm16", "pcm_ext", "is_noise", "is_comfort_noise")):
    """two tuples of per-row outputs, bit for bit; the message names the output (names=None: its index) and the rows"""
    for k, (x, y) in enumerate(zip(got, want)):
        x, y = np.asarray(x), np.asarray(y)
        what = f"output {k}" if names is None else names[k]
        assert np.array_equal(x, y), f"{where}: {what} differs in rows {np.flatnonzero((x != y).reshape(len(x), -1).any(axis=1)).tolist()[:64]}"


def make_ctx(max_streams, mode="xnnpack", rate=None, cng_seed=None, **kw):
    """a context on device 0; rate (the encoder's, for DTX) and cng_seed stay the library's defaults when None; **kw: LyraHip's"""
    import lyra_amd
    c = lyra_amd.LyraHip(device=0, max_streams=max_streams, requant=mode, **kw)
    if rate is not None:
        c.set_encoder_sample_rate(rate)
    if cng_seed is not None:
        c.set_cng_seed(cng_seed)
    return c
