"""The restated libm of the kernels, evaluated ON THE DEVICE (pslfe_debug_math: the product's headers built with the product's flags),
against the host compile of the same headers (oracle/math_oracle.cpp) on the argument grids of tests/math_grids.py: the same bytes,
no tolerance - both sides are the same sequence of single IEEE operations.  tests/test_debug_math_cpu.py checks the grids and the twins
without a GPU."""
import ctypes as C

import numpy as np
import pytest

import math_grids
import oracle_lib

pytestmark = pytest.mark.gpu


def _bits(o):
    return o.view(np.uint32 if o.itemsize == 4 else np.uint64)


@pytest.mark.parametrize("name", sorted(math_grids.GRIDS))
def test_device_equals_host_twin(name, ctx):
    import psl_slam_amd as P
    fn = math_grids.GRIDS[name]
    a, b, distinct = math_grids.grid(name)
    ref = oracle_lib.math_eval(fn, a, b)
    got = P.debug_math(fn, a, b, ctx=ctx)
    ref = ref if isinstance(ref, tuple) else (ref,)
    got = got if isinstance(got, tuple) else (got,)
    assert len(ref) == len(got)
    for which, (r, g) in enumerate(zip(ref, got)):
        assert r.dtype == g.dtype and r.shape == g.shape
        # a NaN result (0 * inf in a quotient) is a NaN on both sides; its sign and payload are no part of the contract
        rb, gb = _bits(r), _bits(g)
        if r.dtype.kind == "f":
            both_nan = np.isnan(r) & np.isnan(g)
            assert both_nan.sum() <= len(r) // 100
        else:
            both_nan = np.zeros(len(r), bool)
        bad = np.flatnonzero((rb != gb) & ~both_nan)
        print(f"{name} out{which}: {len(a)} arguments, {len(np.unique(gb))} distinct outputs, {len(bad)} differ")
        assert len(np.unique(gb)) >= distinct, f"{name}: degenerate outputs"
        if len(bad):
            i = bad[:8]
            a_, b_ = np.ascontiguousarray(a, P.MATH_SIGNATURES[fn][0]), None if b is None else np.ascontiguousarray(b, P.MATH_SIGNATURES[fn][0])
            show = [(a_[j].item().hex() if a_.dtype.kind == "f" else a_[j], None if b_ is None else b_[j].item().hex(), hex(int(gb[j])), hex(int(rb[j]))) for j in i]
            raise AssertionError(f"{name} out{which}: {len(bad)} of {len(a)} differ from the host twin; (a, b, device, host): {show}")


def test_log_gamma_on_the_device_is_the_oracles(ctx):
    """... and for every integer 1 .. 70000 the bytes of the oracle's own log_gamma over the restated functions, which is what the
    reference values of tests/test_nfa_direct_gpu.py are computed with"""
    import psl_slam_amd as P
    x = np.arange(1, 70001, dtype=np.float64)
    old = oracle_lib.set_nfa_math(1)
    try:
        ref = oracle_lib.lsd_log_gamma(x)
    finally:
        oracle_lib.set_nfa_math(old)
    assert P.debug_math("log_gamma", x, ctx=ctx).tobytes() == ref.tobytes()


def test_arguments_are_checked(ctx):
    import psl_slam_amd as P
    lib = P.lib()
    a, o = np.ones(4, np.float32), np.zeros(4, np.float32)
    pa, po = C.c_void_p(a.ctypes.data), C.c_void_p(o.ctypes.data)
    assert lib.pslfe_debug_math(ctx._h, 99, C.c_size_t(4), pa, None, po, None) == -1 and b"unknown function" in lib.pslfe_last_error()
    assert lib.pslfe_debug_math(ctx._h, -1, C.c_size_t(4), pa, None, po, None) == -1
    assert lib.pslfe_debug_math(ctx._h, 0, C.c_size_t(4), None, None, po, None) == -1
    assert lib.pslfe_debug_math(ctx._h, 0, C.c_size_t(4), pa, None, None, None) == -1
    assert lib.pslfe_debug_math(ctx._h, 3, C.c_size_t(4), pa, None, po, None) == -1     # fast_atan2 reads b
    assert lib.pslfe_debug_math(ctx._h, 2, C.c_size_t(4), pa, None, po, None) == -1     # sincosf writes out1
    assert lib.pslfe_debug_math(ctx._h, 0, C.c_size_t(0), None, None, None, None) == 0
    assert P.debug_math("atanf", np.zeros(0, np.float32), ctx=ctx).shape == (0,)
    assert P.debug_math("atanf", np.float32([1.0]), ctx=ctx)[0] == np.float32(np.pi / 4)
