"""CPU tests of the structural operations on resident matrices (spasm_amd_dcsr_transpose / _permute / _vcat / _hcat, DeviceCSR.T,
.transpose(), .permute(), vcat, hcat): symbols, bindings, the header, the argument checks that happen in Python before any C call,
and the loud failure without a device.  Nothing here needs a GPU."""
import contextlib
import ctypes as C
import os
import re

import numpy as np
import pytest

RESHAPE_SYMBOLS = ["spasm_amd_dcsr_transpose", "spasm_amd_dcsr_permute", "spasm_amd_dcsr_vcat", "spasm_amd_dcsr_hcat"]
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spasm_amd.h")


def test_reshape_symbols_exported_bound_and_declared(S):
    lib = S._abi.lib()
    with open(HEADER) as fh:
        text = fh.read()
    for name in RESHAPE_SYMBOLS:
        assert name in S._abi.SIGNATURES, name
        fn = getattr(lib, name)  # exported
        assert fn.argtypes == S._abi.SIGNATURES[name][1] and fn.restype == C.c_void_p, name
        assert re.search(r"spasm_amd_dcsr \*" + name + r"\(", text), name
    assert S._abi.SIGNATURES["spasm_amd_dcsr_permute"][1] == [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    assert S._abi.SIGNATURES["spasm_amd_dcsr_vcat"][1] == S._abi.SIGNATURES["spasm_amd_dcsr_hcat"][1] == [C.c_int32, C.POINTER(C.c_void_p)]
    assert isinstance(S.DeviceCSR.T, property)
    for name in ("transpose", "permute", "vcat", "hcat"):
        assert callable(getattr(S.DeviceCSR, name)), name
    assert callable(S.vcat) and callable(S.hcat) and "vcat" in S.__all__ and "hcat" in S.__all__
    # the statistics keep their names; the docstring says what they mean for the new operations
    assert len(S.DeviceCSR.STATS) == 12 and S.DeviceCSR.STATS[10] == "op"
    assert "4 transpose" in S.DeviceCSR.__doc__


@contextlib.contextmanager
def fake_handles(S, monkeypatch, *specs):
    """DeviceCSR objects of the given (shape, prime) around a handle that must never reach the library: every dcsr entry is
    trapped while they live"""
    class Trap:
        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, name):
            if name.startswith("spasm_amd_dcsr_"):
                raise AssertionError(f"{name} reached")
            return getattr(self._lib, name)

    real = S._abi.lib()
    made = []
    with monkeypatch.context() as mp:
        mp.setattr(S._abi, "lib", lambda: Trap(real))
        try:
            for shape, prime in specs:
                d = object.__new__(S.DeviceCSR)
                d._h, d.shape, d.nnz, d.prime = 0xDEAD0, shape, 0, prime
                made.append(d)
            yield made
        finally:
            for d in made:
                d._h = None  # nothing to free


def test_bad_permutations_rejected_in_python_before_any_c_call(S, monkeypatch):
    with fake_handles(S, monkeypatch, ((4, 3), 127)) as (d,):
        bad_p = [[0, 1, 2, 2], [0, 1, 2, 4], [-1, 0, 1, 2], [0, 1, 2], [0, 1, 2, 3, 4], [[0, 1], [2, 3]], [0.0, 1.0, 2.0, 3.0], [True, False, True, False]]
        for p in bad_p:
            with pytest.raises(ValueError):
                d.permute(p)
            with pytest.raises(ValueError):
                d.permute(p=np.array(p))
        for q in ([0, 0, 1], [0, 1, 3], [0, 1], [2, 1, -1], [0, 1, 2, 3]):
            with pytest.raises(ValueError):
                d.permute(None, q)
            with pytest.raises(ValueError):
                d.permute(qinv=q)
            with pytest.raises(ValueError):
                d.permute([3, 2, 1, 0], q)
        # a good p does not rescue a bad q, and the other way round
        with pytest.raises(ValueError):
            d.permute([0, 1, 2, 2], [2, 1, 0])
        with pytest.raises(ValueError, match="both"):
            d.permute([3, 2, 1, 0], [2, 1, 0], qinv=[2, 1, 0])
        with pytest.raises(ValueError, match="both"):
            d.permute(q=[2, 1, 0], qinv=[0, 1, 2])
        # good arguments do reach the library (the trap says so)
        with pytest.raises(AssertionError, match="spasm_amd_dcsr_permute reached"):
            d.permute([3, 2, 1, 0], [2, 0, 1])
        with pytest.raises(AssertionError, match="spasm_amd_dcsr_transpose reached"):
            d.T


def test_cat_mismatches_rejected_in_python_before_any_c_call(S, monkeypatch):
    specs = (((4, 3), 127), ((5, 3), 127), ((4, 6), 127), ((4, 3), 65521), ((5, 6), 127))
    with fake_handles(S, monkeypatch, *specs) as (a, tall, wide, other_prime, both):
        for call in (lambda: S.vcat(a, wide), lambda: a.vcat(wide), lambda: S.vcat(a, tall, both), lambda: S.hcat(a, tall), lambda: a.hcat(tall),
                     lambda: S.hcat(a, wide, both), lambda: S.vcat(a, other_prime), lambda: S.hcat(a, other_prime), lambda: a.vcat(a, other_prime),
                     lambda: a.hcat(other_prime, a), lambda: S.vcat(), lambda: S.hcat()):
            with pytest.raises(ValueError):
                call()
        A = S.CSR.from_rows([[(0, 1)], [], [], []], 3, prime=127)
        for call in (lambda: S.vcat(a, A), lambda: S.hcat(A, a), lambda: a.vcat(np.zeros((4, 3))), lambda: a.hcat(None), lambda: S.vcat(A), lambda: S.hcat([a, a]),
                     lambda: S.vcat(a, 3)):
            with pytest.raises(TypeError):
                call()
        # shapes that fit do reach the library
        with pytest.raises(AssertionError, match="spasm_amd_dcsr_vcat reached"):
            S.vcat(a, tall)
        with pytest.raises(AssertionError, match="spasm_amd_dcsr_hcat reached"):
            a.hcat(wide)
    # a closed matrix is refused as everywhere
    d = object.__new__(S.DeviceCSR)
    d._h, d.shape, d.nnz, d.prime = None, (4, 3), 0, 127
    for call in (lambda: d.T, lambda: d.transpose(), lambda: d.permute(), lambda: S.vcat(d), lambda: d.hcat(d)):
        with pytest.raises(S.SpasmError, match="closed"):
            call()


def test_reshape_fails_loudly_without_gpu(S):
    """NULL arguments: without a device every entry says "no HIP device" before it looks at them; with one, it refuses them"""
    lib = S._abi.lib()
    want = "no HIP device" if lib.spasm_amd_device_count() <= 0 else "NULL"
    none = (C.c_void_p * 1)(None)
    ident = (C.c_int32 * 3)(0, 1, 2)
    calls = {
        "spasm_amd_dcsr_transpose": lambda: lib.spasm_amd_dcsr_transpose(None),
        "spasm_amd_dcsr_permute": lambda: lib.spasm_amd_dcsr_permute(None, ident, ident),
        "spasm_amd_dcsr_vcat": lambda: lib.spasm_amd_dcsr_vcat(1, none),
        "spasm_amd_dcsr_hcat": lambda: lib.spasm_amd_dcsr_hcat(1, none),
    }
    for name, call in calls.items():
        assert not call(), name
        assert want in S._abi.last_error() and name in S._abi.last_error(), S._abi.last_error()
    want = "no HIP device" if want != "NULL" else "at least one"
    assert not lib.spasm_amd_dcsr_vcat(0, None) and want in S._abi.last_error()
    assert not lib.spasm_amd_dcsr_hcat(-1, None) and want in S._abi.last_error()
