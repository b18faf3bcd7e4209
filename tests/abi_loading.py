"""Loading the C-ABI library and reading its headers, for the CPU tests of the ABI.  No tests, no fixtures (each module's `lib`
fixture calls load_library)."""
import ctypes
import os
import re

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def load_library(raw=False):
    """The library, built first where it is missing: the codec's own handle (codec._load(), every signature table applied), or
    raw: a plain ctypes.CDLL without prototypes, behind a `make` that runs every time."""
    from lyra_amd import codec
    if raw or not os.path.isfile(codec.library_path()):
        codec.build_library()
    return ctypes.CDLL(codec.library_path()) if raw else codec._load()


def _protos(header):
    """name -> parameter list as text, of every `int lyra_hip_*(...)` prototype of include/<header>, comments dropped"""
    hdr = open(os.path.join(ROOT, "include", header)).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(lyra_hip_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)}
