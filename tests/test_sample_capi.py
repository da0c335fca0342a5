"""The argument rules of pli_sample (include/pli.h) without a GPU: every rule
returns its status with its message before any HIP call (the data pointers are
never dereferenced, nothing is launched), the workspace size is 0 for every
shape, and the binding declares the header's signature."""
from __future__ import annotations

import ctypes
import os
import re

import pytest

import sample_cases as sc
from conftest import ROOT

OK, EINVAL, EUNSUPPORTED = 0, 1000, 1001
F32, F16, BF16 = 0, 1, 2
P = 4096        # never dereferenced: validation fails first
ODD = 4104      # 8 bytes past a 16-byte boundary


@pytest.fixture()
def L(built_lib):
    import pli_hip
    return pli_hip.lib()


def _sample(L, **kw):
    a = dict(logits=P, ld=64, rows=4, vocab=64, dtype=BF16, t=1.0, k=0, p=1.0, uniforms=None, seed=0, od=None, oa=0,
             tokens=P, ldt=1, ws=None, wsb=0)
    a.update(kw)
    return L.pli_sample(a["logits"], a["ld"], a["rows"], a["vocab"], a["dtype"], a["t"], a["k"], a["p"], a["uniforms"],
                        a["seed"], a["od"], a["oa"], a["tokens"], a["ldt"], a["ws"], a["wsb"], None)


def test_symbols_declared_and_exported(L):
    header = " ".join(open(os.path.join(ROOT, "include", "pli.h")).read().split())
    assert "size_t pli_sample_workspace_size(int rows, int vocab, int dtype);" in header
    assert re.search(r"\bint pli_sample\(const void\* logits, int64_t ld_logits, int rows, int vocab, int dtype, "
                     r"float temperature, int top_k, float top_p, const float\* uniforms, uint64_t seed, "
                     r"const int32_t\* offset_dev, int64_t offset_add, int64_t\* tokens, int64_t ld_tokens, "
                     r"void\* workspace, size_t workspace_bytes, void\* stream\);", header)
    assert L.pli_sample.argtypes[9] is ctypes.c_uint64 and L.pli_sample_workspace_size.restype is ctypes.c_size_t
    assert f"vocab <= {sc.MAX_VOCAB}" in header


def test_workspace_size_is_zero(L):
    for rows, vocab, dt in ((1, 1, F32), (33, 32000, BF16), (1, 128256, F16), (4096, sc.MAX_VOCAB, F32)):
        assert L.pli_sample_workspace_size(rows, vocab, dt) == 0


def test_sample_argument_rules_without_gpu(L):
    err = L.pli_last_error
    nan, inf = float("nan"), float("inf")
    for kw in (dict(rows=-1), dict(vocab=0), dict(vocab=-5), dict(ld=63), dict(ld=0), dict(ldt=0), dict(ldt=-1)):
        assert _sample(L, **kw) == EINVAL and b"pli_sample: bad shape" in err(), kw
    assert b"rows=4 vocab=64 ld_logits=64 ld_tokens=-1" in err()
    for dt in (3, 7, -1):
        assert _sample(L, dtype=dt) == EINVAL and b"pli_sample: bad dtype" in err(), dt
    for kw in (dict(t=-1.0), dict(t=-0.5, k=3), dict(t=nan), dict(p=-0.1), dict(p=nan), dict(t=-inf), dict(p=-inf)):
        assert _sample(L, **kw) == EINVAL and b"temperature and top_p must be >= 0 and not NaN" in err(), kw
    assert _sample(L, ws=ODD, wsb=1024) == EINVAL and b"workspace too small or not 16-byte aligned" in err()
    for name in ("logits", "tokens"):
        assert _sample(L, **{name: None}) == EINVAL and b"pli_sample: null pointer" in err(), name
    # the rules hold for the greedy instance too (temperature 0 is valid; its other arguments are still checked)
    assert _sample(L, t=0.0, logits=None) == EINVAL and b"null pointer" in err()
    assert _sample(L, t=0.0, p=nan) == EINVAL and b"top_p" in err()
    assert L.pli_last_route() == b""   # nothing was launched


def test_vocab_limit_is_unsupported_not_invalid(L):
    v = sc.MAX_VOCAB + 1
    assert _sample(L, vocab=v, ld=v) == EUNSUPPORTED
    assert b"pli_sample: vocab=%d above the supported %d" % (v, sc.MAX_VOCAB) in L.pli_last_error()
    assert _sample(L, vocab=v, ld=v - 1) == EINVAL   # (a bad shape is still a bad shape)
    assert L.pli_last_route() == b""


def test_empty_call_does_nothing(L):
    """rows == 0: PLI_OK, operands may be NULL, no launch; the argument rules still come first"""
    assert _sample(L, rows=0, logits=None, tokens=None) == OK
    assert L.pli_last_error() == b"" and L.pli_last_route() == b""
    assert _sample(L, rows=0, ws=P, wsb=64, uniforms=None, od=None) == OK
    assert _sample(L, rows=0, t=-1.0) == EINVAL and _sample(L, rows=0, dtype=9) == EINVAL
    assert _sample(L, rows=0, vocab=sc.MAX_VOCAB + 1, ld=sc.MAX_VOCAB + 1) == EUNSUPPORTED
