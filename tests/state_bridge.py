"""Bridge between the CPU oracle's per-stream state (oracle/lyra_oracle.py Stream.state()) and the product's stream blob
(lyra_amd/csrc/stream_blob.h, state_layout.h): the 32 tensors of the six stage regions R_E0 .. R_D2, and M_PREV of R_MEL.

A plain helper module for tests/test_state_bridge_cpu.py and tests/test_gpu_state_vs_oracle.py.  It restates the DOCUMENTED
layout, independently of the kernels that write it:

  * the oracle keeps a history as a shift buffer [R rows][C channels], oldest row first, channels in the graph's order;
  * the blob keeps a history whose R rows outlast one hop's T new rows (T < R) as a RING: oracle row j lies at ring row
    (phase * T + j) mod R, phase = frames the side has processed mod 18, kept in the first word of the region's slot;
    a history with T >= R is replaced every hop and lies oldest row first;
  * fp32 rows of the MFMA stages are in AT16 channel order (inside every aligned block of 16 channels the 4 x 4 index matrix
    is transposed: channel k lies at (k & ~15) | ((k & 3) << 2) | ((k >> 2) & 3)); the tails of the transposed convolutions,
    the first conv's sample history and all int8 rows are in natural order;
  * a tensor inside an int8 part of a graph is held as int8 CODES with its producer's scale s and zero point z (weight
    container entries named in the table); the oracle holds the floats DEQUANTIZE gives.  The dequantisation used here is
    the oracle's dequantize_f:  float32(float64(s) * float64(code - z)).  Going from floats to codes is only right when
    it loses nothing, so to_blob asserts dequantize(code) == float BIT FOR BIT on every element, whatever the mode;
  * M_PREV is the previous hop as int16; the oracle keeps the same samples as doubles;
  * every byte of those regions that is neither a tensor nor a phase word is padding and zero.

Region offsets and sizes come from tests/stream_state/blob_tool.cc compiled over stream_blob.h (`layout`, `tensors`), as
tests/test_stream_state_cpu.py takes them; nothing of the layout is a literal here except the SHAPES of the table.
"""
import json
import os
import struct
import subprocess

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "lyra_amd", "csrc")
PACK = os.path.join(ROOT, "lyra_amd", "assets", "lyra_v1.lyrapack")
MODES = {"exact": 0, "gemmlowp_double": 1, "xnnpack": 2, "builtin_mixed": 3}
R_E0, R_E1, R_E2, R_D0, R_D1, R_D2, R_MEL = range(7)
ENC_REGIONS, DEC_REGIONS = (R_E0, R_E1, R_E2), (R_D0, R_D1, R_D2)
PHASED = (R_E1, R_E2, R_D0, R_D1)          # regions that hold a ring, hence a phase word

# name, region, offset constant of state_layout.h (+ bytes), dtype, rows R, channels C, rows per hop T, channel order,
# (weight-container entry, index of the scale in it) of an int8 tensor's producer.  ring <=> T < R.
_T = [
    ("e_first", R_E0, "E_FIRST", 0, "f32", 1, 48, 1, "natural", None),       # 48 samples, replaced every hop
    ("e_r0[0]", R_E0, "E_R0_0", 0, "f32", 2, 64, 20, "at16", None),
    ("e_r0[1]", R_E0, "E_R0_1", 0, "f32", 6, 64, 20, "at16", None),
    ("e_r0[2]", R_E0, "E_R0_2", 0, "f32", 18, 64, 20, "at16", None),
    ("e_d0", R_E0, "E_D0", 0, "f32", 5, 64, 20, "at16", None),
    ("e_r1[0]", R_E1, "E_R1_0", 0, "f32", 2, 128, 4, "at16", None),
    ("e_r1[1]", R_E1, "E_R1_1", 0, "f32", 6, 128, 4, "at16", None),
    ("e_r1[2]", R_E1, "E_R1_2", 0, "f32", 18, 128, 4, "at16", None),
    ("e_d1", R_E1, "E_D1", 0, "f32", 2, 128, 4, "at16", None),
    ("e_r2[0]", R_E2, "E_R2_0", 0, "f32", 2, 256, 2, "at16", None),
    ("e_r2[1]", R_E2, "E_R2_1", 0, "i8", 6, 256, 2, "natural", ("enc.lrelu8.1.q", 2)),
    ("e_r2[2]", R_E2, "E_R2_2", 0, "i8", 18, 256, 2, "natural", ("enc.lrelu8.3.q", 2)),
    ("e_d2", R_E2, "E_D2", 0, "i8", 2, 256, 2, "natural", ("enc.lrelu8.5.q", 2)),
    ("e_bott", R_E2, "E_BOTT", 0, "i8", 2, 512, 1, "natural", ("enc.lrelu8.6.q", 2)),
    ("d_head", R_D0, "D_HEAD", 0, "f32", 2, 64, 1, "at16", None),
    ("d_up0[0]", R_D0, "D_UP0", 0 * 512, "f32", 2, 64, 2, "natural", None),
    ("d_up0[1]", R_D0, "D_UP0", 1 * 512, "f32", 2, 64, 2, "natural", None),
    ("d_up0[2]", R_D0, "D_UP0", 2 * 512, "f32", 2, 64, 2, "natural", None),
    ("d_up0[3]", R_D0, "D_UP0", 3 * 512, "f32", 2, 64, 2, "natural", None),
    ("d_r0[0]", R_D0, "D_R0_0", 0, "i8", 2, 256, 2, "natural", ("dec.quant.1.q", 0)),
    ("d_r0[1]", R_D0, "D_R0_1", 0, "i8", 6, 256, 2, "natural", ("dec.lrelu8.1.q", 2)),
    ("d_r0[2]", R_D0, "D_R0_2", 0, "i8", 18, 256, 2, "natural", ("dec.lrelu8.3.q", 2)),
    ("d_up1[0]", R_D0, "D_UP1", 0 * 512, "f32", 2, 64, 2, "natural", None),
    ("d_up1[1]", R_D0, "D_UP1", 1 * 512, "f32", 2, 64, 2, "natural", None),
    ("d_r1[0]", R_D1, "D_R1_0", 0, "f32", 2, 128, 4, "at16", None),
    ("d_r1[1]", R_D1, "D_R1_1", 0, "f32", 6, 128, 4, "at16", None),
    ("d_r1[2]", R_D1, "D_R1_2", 0, "f32", 18, 128, 4, "at16", None),
    ("d_up2", R_D1, "D_UP2", 0, "f32", 5, 64, 5, "natural", None),
    ("d_r2[0]", R_D2, "D_R2_0", 0, "f32", 2, 64, 20, "at16", None),
    ("d_r2[1]", R_D2, "D_R2_1", 0, "f32", 6, 64, 20, "at16", None),
    ("d_r2[2]", R_D2, "D_R2_2", 0, "f32", 18, 64, 20, "at16", None),
    ("d_up3", R_D2, "D_UP3", 0, "f32", 1, 48, 1, "natural", None),            # 48 samples of tail, replaced every hop
    ("mel_prev", R_MEL, "M_PREV", 0, "i16", 1, 320, 1, "natural", None),
]


class Tensor:
    def __init__(self, row, tensors, pack):
        self.name, self.region, key, extra, self.dtype, self.R, self.C, self.T, order, q = row
        self.off = tensors[key] + extra                     # inside the region's slot
        self.ring = self.T < self.R
        self.at16 = order == "at16"
        self.itemsize = {"f32": 4, "i8": 1, "i16": 2}[self.dtype]
        self.nbytes = self.R * self.C * self.itemsize
        self.scale = self.zero = None
        if q is not None:
            v = pack[q[0]]
            self.scale, self.zero = np.float32(v[q[1]]), int(v[q[1] + 1])
            assert float(v[q[1] + 1]) == self.zero and -128 <= self.zero <= 127, f"{self.name}: zero point {v[q[1] + 1]} is no int8 code"

    @property
    def side(self):
        return "enc" if self.region in ENC_REGIONS or self.region == R_MEL else "dec"


def read_pack(path=PACK):
    """name -> float32 array of every `.q` entry of the weight container (pack_format.h: 16-byte header, 96-byte entries)"""
    raw = open(path, "rb").read()
    assert raw[:8] == b"LYRAPK01", f"{path}: begins with {raw[:8]!r}, not with the weight pack's magic"
    out = {}
    for i in range(struct.unpack_from("<I", raw, 8)[0]):
        off = 16 + 96 * i
        name = raw[off:off + 56].split(b"\0")[0].decode()
        o, nb = struct.unpack_from("<2Q", raw, off + 80)
        if name.endswith(".q"):
            out[name] = np.frombuffer(raw, np.float32, nb // 4, o).copy()
    return out


def compile_tool(directory):
    exe = os.path.join(str(directory), "blob_tool")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", CSRC,
                           os.path.join(ROOT, "tests", "stream_state", "blob_tool.cc"), "-o", exe])
    return exe


def _verdicts(tool, tmp_path, blobs, mode=MODES["xnnpack"]):
    """blob_tool's validate() verdict per blob"""
    path = str(tmp_path / "blobs.bin")
    np.ascontiguousarray(blobs, np.uint8).tofile(path)
    return [int(x) for x in subprocess.check_output([tool, "validate", path, str(mode)]).split()]


def _reset_blob(tool, tmp_path, mode=MODES["xnnpack"]):
    """the blob of a freshly reset stream, as blob_tool writes it"""
    path = str(tmp_path / "reset.bin")
    subprocess.check_call([tool, "reset", path, str(mode)])
    return np.fromfile(path, np.uint8)


def at16(k):
    k = np.asarray(k)
    return (k & ~15) | ((k & 3) << 2) | ((k >> 2) & 3)


def dequantize(codes, scale, zero):
    """the oracle's dequantize_f: float32(float64(s) * float64(code - z))"""
    return (np.float64(scale) * (np.asarray(codes, np.int64) - zero).astype(np.float64)).astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class Bridge:
    def __init__(self, tool):
        """tool: path of the compiled tests/stream_state/blob_tool.cc"""
        self.L = json.loads(subprocess.check_output([tool, "layout"]))
        self.K = json.loads(subprocess.check_output([tool, "tensors"]))
        pack = read_pack()
        self.tensors = [Tensor(r, self.K, pack) for r in _T]
        self.by_name = {t.name: t for t in self.tensors}
        self.bytes = self.L["bytes"]
        self.phase_mod = self.K["PHASE_MOD"]

    def region(self, r):
        """(offset in the blob, bytes) of region r"""
        return tuple(self.L["pieces"][r])

    def phase_off(self, r):
        return self.region(r)[0] + self.K["PHASE"]

    def span(self, t):
        o = self.region(t.region)[0] + t.off
        return o, o + t.nbytes

    def phases(self, blob):
        """region -> its phase word"""
        return {r: int(np.frombuffer(blob[self.phase_off(r):self.phase_off(r) + 4].tobytes(), "<u4")[0]) for r in PHASED}

    def use_count(self):
        """per byte of a blob: how many table tensors or phase words claim it"""
        use = np.zeros(self.bytes, np.int32)
        for t in self.tensors:
            a, b = self.span(t)
            use[a:b] += 1
        for r in PHASED:
            use[self.phase_off(r):self.phase_off(r) + 4] += 1
        return use

    def scope(self):
        """bool per byte of a blob: inside the six stage regions or M_PREV's extent (what to_blob writes and checks)"""
        m = np.zeros(self.bytes, bool)
        for r in ENC_REGIONS + DEC_REGIONS:
            o, n = self.region(r)
            m[o:o + n] = True
        a, b = self.span(self.by_name["mel_prev"])
        m[a:b] = True
        return m

    def padding(self):
        return self.scope() & (self.use_count() == 0)

    # ---- one tensor -----------------------------------------------------------------------------------------------------
    def _rows_to_blob(self, t, rows, phase):
        """rows [R][C] in the oracle's order -> the tensor's [R][C] as the blob holds it"""
        out = rows
        if t.at16:
            phys = np.empty_like(rows)
            phys[:, at16(np.arange(t.C))] = rows
            out = phys
        if t.ring:
            ring = np.empty_like(out)
            ring[(phase * t.T + np.arange(t.R)) % t.R] = out
            out = ring
        return out

    def _rows_from_blob(self, t, rows, phase):
        out = rows
        if t.ring:
            out = out[(phase * t.T + np.arange(t.R)) % t.R]
        if t.at16:
            out = out[:, at16(np.arange(t.C))]
        return out

    def codes_of(self, t, x):
        """floats -> the tensor's stored integers, asserting that nothing is lost"""
        x = np.ascontiguousarray(x)
        if t.dtype == "i16":
            c = np.rint(x).astype(np.int64)
            assert np.array_equal(c.astype(np.float64), x) and c.min() >= -32768 and c.max() <= 32767, f"{t.name}: not int16 samples"
            return c.astype(np.int16)
        c = np.rint(x.astype(np.float64) / np.float64(t.scale)).astype(np.int64) + t.zero
        bad = (c < -128) | (c > 127) | (_bits(dequantize(np.clip(c, -128, 127), t.scale, t.zero)) != _bits(x))
        if bad.any():
            i = int(np.flatnonzero(bad.ravel())[0])
            raise AssertionError(f"{t.name}: element {i} = {x.ravel()[i]!r} is no code of scale {t.scale!r}, zero {t.zero} "
                                 f"(nearest code {int(c.ravel()[i])} -> {dequantize(np.clip(c.ravel()[i], -128, 127), t.scale, t.zero)!r})")
        return c.astype(np.int8)

    def floats_of(self, t, c):
        if t.dtype == "i16":
            return c.astype(np.float64)
        return dequantize(c, t.scale, t.zero)

    # ---- whole blobs ----------------------------------------------------------------------------------------------------
    def to_blob(self, state, frames_enc, frames_dec, mode, header_from):
        """oracle state (dict of Stream.state()) -> a blob: header and every region outside the table's scope are those of
        `header_from` (a blob of the target, e.g. a reset export); the six stage regions and M_PREV are built from `state`,
        the phase words from the frame counts, padding zero."""
        blob = np.array(header_from, np.uint8).copy()
        assert blob.shape == (self.bytes,), f"a blob of shape {blob.shape}, not of {self.bytes} bytes"
        h = self.L["h"]["mode"]
        assert int(np.frombuffer(blob[h:h + 4].tobytes(), "<u4")[0]) == MODES[mode], "header_from is of another mode"
        blob[self.scope()] = 0
        ph = {R_E1: frames_enc % self.phase_mod, R_E2: frames_enc % self.phase_mod,
              R_D0: frames_dec % self.phase_mod, R_D1: frames_dec % self.phase_mod}
        for r, p in ph.items():
            blob[self.phase_off(r):self.phase_off(r) + 4] = np.frombuffer(struct.pack("<I", p), np.uint8)
        for t in self.tensors:
            x = np.asarray(state[t.name]).reshape(t.R, t.C)
            stored = x.astype(np.float32) if t.dtype == "f32" else self.codes_of(t, x)
            if t.dtype == "f32":
                assert np.array_equal(_bits(stored), _bits(x)), f"{t.name}: float32 state changes when stored as float32"
            a, b = self.span(t)
            blob[a:b] = np.ascontiguousarray(self._rows_to_blob(t, stored, ph.get(t.region, 0))).view(np.uint8).ravel()
        return blob

    def from_blob(self, blob):
        """a blob -> oracle state (dict as Stream.state(): flat arrays, float32, mel_prev float64)"""
        blob = np.ascontiguousarray(blob, np.uint8)
        assert blob.shape == (self.bytes,), f"a blob of shape {blob.shape}, not of {self.bytes} bytes"
        ph = self.phases(blob)
        np_t = {"f32": "<f4", "i8": np.int8, "i16": "<i2"}
        out = {}
        for t in self.tensors:
            a, b = self.span(t)
            rows = np.frombuffer(blob[a:b].tobytes(), np_t[t.dtype]).reshape(t.R, t.C)
            rows = self._rows_from_blob(t, rows, ph.get(t.region, 0) % self.phase_mod)
            out[t.name] = (rows.astype(np.float32) if t.dtype == "f32" else self.floats_of(t, rows)).ravel().copy()
        return out

    # ---- comparison -----------------------------------------------------------------------------------------------------
    def first_difference(self, got, want):
        """None, or a sentence naming the first tensor (table order) whose bits differ, its first differing row and channel
        (oracle order) and both values; got / want: dicts as from_blob / Stream.state() give"""
        for t in self.tensors:
            g, w = np.asarray(got[t.name]).reshape(t.R, t.C), np.asarray(want[t.name]).reshape(t.R, t.C)
            if t.dtype == "i16":
                d = g != w
            else:
                d = _bits(g) != _bits(w)
            if d.any():
                r, c = (int(v) for v in np.argwhere(d)[0])
                extra = ""
                if t.scale is not None:
                    extra = (f" (codes {int(np.rint(np.float64(g[r, c]) / np.float64(t.scale))) + t.zero} / "
                             f"{int(np.rint(np.float64(w[r, c]) / np.float64(t.scale))) + t.zero})")
                return (f"tensor {t.name}: {int(d.sum())} of {d.size} elements differ, first at row {r} channel {c}: "
                        f"got {g[r, c]!r}, oracle {w[r, c]!r}{extra}")
        return None
