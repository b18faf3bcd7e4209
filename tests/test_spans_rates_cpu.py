"""CPU: what the span calls with per-span sample rates rest on (include/lyra_hip_spans_rates.h; DESIGN.md 4.5 "Per-span sample
rates").  The new header, the third ctypes table of lyra_amd/codec.py (_SIGNATURES_SPANS_RATES) and the built library agree on
the three symbols; a null context is refused by all three; LyraHip has the three methods; include/lyra_hip.h, _SIGNATURES and
the mixed header keep their counts, and neither older header pulls the new one in."""
import os
import re

import pytest

from lyra_amd import codec

from abi_loading import _protos, load_library

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW = {"lyra_hip_encode_spans_rates_dev": 12, "lyra_hip_decode_spans_lossy_rates_dev": 12, "lyra_hip_decode_spans_rates_dev": 10}


@pytest.fixture(scope="module")
def lib():
    return load_library()


def test_header_third_table_and_library_agree_on_the_three_symbols(lib):
    protos = _protos("lyra_hip_spans_rates.h")
    assert set(protos) == set(NEW) == set(codec._SIGNATURES_SPANS_RATES)
    for name, n_args in NEW.items():
        args = [a.strip() for a in protos[name].split(",")]
        assert len(args) == n_args, (name, args)
        fn = getattr(lib, name, None)
        assert fn is not None, f"{name} is not exported by {codec.library_path()}"
        restype, argtypes = codec._SIGNATURES_SPANS_RATES[name]
        assert restype is codec.C.c_int and fn.restype is restype and list(fn.argtypes) == list(argtypes), name
        assert len(argtypes) == n_args, (name, argtypes)
        for a, t in zip(args, argtypes):   # pointers as void pointers, everything else an int
            assert ("*" in a) == (t is codec.C.c_void_p), (name, a, t)


def test_a_null_context_is_refused_by_all_three(lib):
    for name, n_args in NEW.items():
        args = [0 if t is codec.C.c_int else None for t in codec._SIGNATURES_SPANS_RATES[name][1]]
        assert len(args) == n_args
        assert getattr(lib, name)(*args) < 0, name


def test_lyrahip_has_the_three_methods():
    for name in NEW:
        assert callable(getattr(codec.LyraHip, name[len("lyra_hip_"):], None)), name


def test_the_older_headers_and_tables_are_what_they_were():
    old = open(os.path.join(ROOT, "include", "lyra_hip.h")).read()
    mixed = open(os.path.join(ROOT, "include", "lyra_hip_spans_mixed.h")).read()
    for text in (old, mixed):
        assert "lyra_hip_spans_rates.h" not in re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert "#include \"lyra_hip_spans_mixed.h\"" in open(os.path.join(ROOT, "include", "lyra_hip_spans_rates.h")).read()
    old = re.sub(r"^[ \t]*#[^\n]*", "", re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", old, flags=re.S)), flags=re.M)
    all_protos = {name for _, name, _ in re.findall(r"([A-Za-z_][\w\s\*]*?)\b(lyra_hip_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", old)}
    assert len(all_protos) == 98, len(all_protos)   # (the parse of tests/test_abi_cpu.py)
    assert len(codec._SIGNATURES) == 88
    assert len(_protos("lyra_hip_spans_mixed.h")) == 5 == len(codec._SIGNATURES_SPANS_MIXED)
    assert not set(NEW) & (set(codec._SIGNATURES) | set(codec._SIGNATURES_SPANS_MIXED) | all_protos)
