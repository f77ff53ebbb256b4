"""The hybrid PRD tables built on the device (lwhip_hprd_build, lightweaver_amd.hprd.build_hprd, Context(hprd=True)):
configure_hprd_coeffs (Source/Prd.cpp:697-946) as four kernels.

GPU: the device's tables equal the oracle's restatement (lworacle_hprd_build, which tests/test_hprd.py pins to the core) bit
for bit -- the build uses only correctly rounded fp64 operations, so there is no tolerance -- over velocities, ray counts,
depth counts, a grid whose ends are PRD-active, a detailed atom's PRD line with and without includeDetailed; and
Context(prob, hprd=True) runs the hybrid iteration to the oracle's results at the one-call bound.
CPU: the refusals, each with its message and *out left NULL, and the ABI."""
import ctypes as C
import functools
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from lightweaver_amd import _abi as abi
from lightweaver_amd import context, model
from lightweaver_amd.harness import models
from oracle import bindings
from tests.helpers import TOL_ONE_CALL, rel_err
from tests.test_hprd import assert_same, assert_tables_equal, hprd_problem, run_hprd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'lwhip.h')


def snapshot(t):
    """Copies of a table set's arrays and sizes (the views die with close())."""
    h = t.ptr.contents
    return SimpleNamespace(NprdLambda=int(h.NprdLambda), NhPrd=int(h.NhPrd), Nlines=int(h.Nlines),
                           prdIdxs=t.prdIdxs.copy(), hPrdIdxs=t.hPrdIdxs.copy(), jCoeffOff=t.jCoeffOff.copy(),
                           jIdx=t.jIdx.copy(), jFrac=t.jFrac.copy(), lineAtom=t.lineAtom.copy(), lineTrans=t.lineTrans.copy(),
                           rho=[(a.copy(), b.copy(), c.copy()) for a, b, c in t.rho])


def assert_same_tables(a, b):
    assert (a.NprdLambda, a.NhPrd, a.Nlines) == (b.NprdLambda, b.NhPrd, b.Nlines)
    assert_tables_equal(a, b)


def oracle_tables(prob, includeDetailed=False):
    with bindings.OracleContext(prob.copy()) as oc:
        t = oc.build_hprd(includeDetailed)
        snap = snapshot(t)
        t.close()
    return snap


def device_tables(prob, includeDetailed=False):
    from lightweaver_amd.hprd import build_hprd
    t = build_hprd(prob.copy(), includeDetailed=includeDetailed)
    assert t is not None
    assert np.array_equal(t.JRest, np.zeros((t.NprdLambda, prob.Nspace)))   # its own zeroed array
    snap = snapshot(t)
    t.close()
    assert t.ptr is None
    return snap


@functools.lru_cache(maxsize=None)
def base_problem(vamp=8.0e3, Nrays=3, Nspace=None):
    return hprd_problem(vamp=vamp, Nrays=Nrays, Nspace=Nspace)


def edge_problem():
    """A grid inside Ca II K: the line covers it from the first wavelength to the last, so both ends are PRD-active (the two
    constant-extrapolation branches, the decreasing tail at idx = Nspect - 1, the roll-back that reaches index 0).  20 km/s of
    both signs move a rest wavelength across four grid intervals."""
    p = base_problem(vamp=20.0e3)
    w = np.linspace(393.2, 393.5, 61)
    chi, eta, sca, alpha = models.observer_grid_inputs(models.falc82(), [models.H_6(0.3), models.CaII_6(0.3, prd=True)], w)
    return model.observer_problem(p, [0.25, 0.7, 1.0], wavelengths=w, background=(chi, eta, sca), contAlpha=alpha)


def detailed_problem():
    """H Lyman-alpha PRD in an active atom, Ca II H & K PRD in a detailed one (tests/test_prd.py), on a moving column."""
    from tests.test_prd import detailed_prd_problem
    p = detailed_prd_problem()
    k = np.arange(p.Nspace)
    p.vlosMu = np.ascontiguousarray(p.muz[:, None] * (12.0e3 * np.sin(2.0 * np.pi * k / 23.0))[None, :])
    return p


# ---- GPU: the tables -----------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize('vamp', [0.0, 8.0e3, 40.0e3])
def test_device_tables_match_oracle_velocities(gpu, vamp):
    """fac == 1 everywhere (every comparison a tie), a few km/s, and 40 km/s where a walk spans many wavelengths."""
    prob = base_problem(vamp=vamp)
    want = oracle_tables(prob)
    assert want.NhPrd >= want.NprdLambda > 0 and want.jIdx.size > 0
    assert_same_tables(device_tables(prob), want)


@pytest.mark.gpu
@pytest.mark.parametrize('Nrays', [1, 3, 5])
def test_device_tables_match_oracle_ray_counts(gpu, Nrays):
    prob = base_problem(Nrays=Nrays)
    assert_same_tables(device_tables(prob), oracle_tables(prob))


@pytest.mark.gpu
@pytest.mark.parametrize('Nspace', [3, 5, 37, 82, 130])
def test_device_tables_match_oracle_depth_counts(gpu, Nspace):
    """Fewer depths than a wavefront, more than one (130: not a multiple of 64)."""
    prob = base_problem(Nspace=Nspace)
    assert prob.Nspace == Nspace
    assert_same_tables(device_tables(prob), oracle_tables(prob))


@pytest.mark.gpu
def test_device_tables_match_oracle_on_a_grid_with_prd_active_ends(gpu):
    prob = edge_problem()
    want = oracle_tables(prob)
    assert want.prdIdxs[0] == 0 and want.prdIdxs[-1] == prob.Nlambda - 1
    assert prob.vlosMu.min() < 0.0 < prob.vlosMu.max()
    assert want.hPrdIdxs[0] == 0 and want.hPrdIdxs[-1] == prob.Nlambda - 1
    # both extrapolation branches are taken: lists of the end wavelengths that carry weight-1 entries
    first, last = want.jCoeffOff[0], want.jCoeffOff[-1]
    ncellPerLa = prob.Nrays * 2 * prob.Nspace
    assert np.any(want.jFrac[first:want.jCoeffOff[ncellPerLa]] == 1.0)
    assert np.any(want.jFrac[want.jCoeffOff[-1 - ncellPerLa]:last] == 1.0)
    assert_same_tables(device_tables(prob), want)


@pytest.mark.gpu
@pytest.mark.parametrize('includeDetailed', [0, 1])
def test_device_tables_match_oracle_with_a_detailed_prd_atom(gpu, includeDetailed):
    prob = detailed_problem()
    want = oracle_tables(prob, includeDetailed)
    assert want.Nlines == (3 if includeDetailed else 1)   # the line lists differ
    assert_same_tables(device_tables(prob, includeDetailed), want)


# ---- GPU: end to end --------------------------------------------------------------------------------------------------------

def run_hprd_device(prob, nIter, prdIter, tol=1e-2):
    """run_hprd's loop through Context(prob, hprd=True): the context builds, owns and frees its tables."""
    from lightweaver_amd.context import Context
    p = prob.copy()
    out = []
    with Context(p, hprd=True) as ctx:
        assert ctx.sweep_kind() == 'lanes'
        tables = ctx.hprd_tables
        snap = snapshot(tables)
        for it in range(nIter):
            p.gamma_prefill()
            ctx.formal_sol_gamma_matrices()
            if it >= 1:
                ctx.stat_equil()
            out.append(ctx.redistribute_prd(prdIter, tol))
        ctx.download(abi.J)
        JRest = tables.JRest.copy()
    assert tables.ptr is None and ctx.hprd_tables is None   # freed with the context
    return p, out, JRest, snap


@pytest.mark.gpu
@pytest.mark.parametrize('nIter,prdIter', [(1, 2), (3, 3)])
def test_context_hprd_true_matches_oracle(gpu, nIter, prdIter):
    """Context(prob, hprd=True) against the oracle run on the oracle's tables: J, I, JRest, rho, Gamma and the rates at the
    one-call bound (not bit equality: Gamma and JRest are summed by atomics).  Measured on an MI355X, J / I / JRest:
    1.6e-11 / 3.6e-11 / 1.0e-11 after 1 x 2, 5.5e-11 / 1.3e-10 / 4.9e-11 after 3 x 3."""
    prob = base_problem()
    po, uo, Jo = run_hprd(bindings.OracleContext, prob, nIter=nIter, prdIter=prdIter)
    ph, uh, Jh, snap = run_hprd_device(prob, nIter, prdIter)
    assert_same_tables(snap, oracle_tables(prob))
    for a, b in zip(uo, uh):
        assert a['NprdSubIter'] == b.NprdSubIter
    errs = {'JRest': rel_err(Jh, Jo), 'J': rel_err(ph.J, po.J), 'I': rel_err(ph.I, po.I)}
    print('hprd=True vs oracle, %d iteration(s) x %d sub-iteration(s):' % (nIter, prdIter), errs)
    assert np.abs(Jo).max() > 0.0
    assert errs['JRest'] <= TOL_ONE_CALL, errs
    assert_same(po, ph, TOL_ONE_CALL)


@pytest.mark.gpu
def test_second_context_after_close_builds_the_same_tables(gpu):
    """Ownership and free: the tables die with their context, and a second Context(hprd=True) of the same problem builds the
    same ones; so does one made with like= (hprd tables are never borrowed)."""
    from lightweaver_amd.context import Context
    prob = base_problem()
    p = prob.copy()
    with Context(p, hprd=True) as a:
        first = snapshot(a.hprd_tables)
    with Context(p, hprd=True) as b:
        assert_same_tables(snapshot(b.hprd_tables), first)
        q = prob.copy()
        with Context(q, hprd=True, like=b) as c:
            assert c.hprd_tables is not b.hprd_tables and c.hprd_tables.ptr
            assert_same_tables(snapshot(c.hprd_tables), first)
            q.gamma_prefill()
            assert c.formal_sol_gamma_matrices().dJMax > 0.0


@pytest.mark.gpu
def test_given_tables_still_work(gpu):
    """hprd=<tables> as before: build_hprd's tables handed to a context, which borrows and does not free them."""
    from lightweaver_amd.context import Context
    from lightweaver_amd.hprd import build_hprd
    p = base_problem().copy()
    with build_hprd(p) as tables:
        with Context(p, hprd=tables) as ctx:
            assert ctx.hprd_tables is tables and ctx.sweep_kind() == 'lanes'
            p.gamma_prefill()
            ctx.formal_sol_gamma_matrices()
            ctx.download(abi.J)
        assert tables.ptr and np.abs(tables.JRest).max() > 0.0


# ---- CPU: refusals and the ABI ----------------------------------------------------------------------------------------------

def plain_problem():
    return models.falc_h_ca(Nrays=3, lineScale=0.3, computeProfiles=False)


@functools.lru_cache(maxsize=None)
def small_prd_problem():
    return models.falc_h_ca(Nrays=3, lineScale=0.3, prd=True, computeProfiles=False)


def call_build(lib, desc, includeDetailed=0):
    """lwhip_hprd_build with *out pointing at something first: a refusal must leave it NULL."""
    dummy = abi.lwhip_hprd()
    out = C.pointer(dummy)
    st = lib.lwhip_hprd_build(C.byref(desc) if desc is not None else None, None, includeDetailed, C.byref(out))
    return st, out, lib.lwhip_last_error().decode()


def test_refuses_null_arguments(hip_lib):
    st, out, msg = call_build(hip_lib, None)
    assert st == abi.ERR_INVALID and not out and 'null problem' in msg
    desc = small_prd_problem().descriptor()
    assert hip_lib.lwhip_hprd_build(C.byref(desc), None, 0, None) == abi.ERR_INVALID
    assert 'null out' in hip_lib.lwhip_last_error().decode()


def test_refuses_abi_mismatch(hip_lib):
    desc = small_prd_problem().descriptor()
    desc.abiVersion = 3
    st, out, msg = call_build(hip_lib, desc)
    assert st == abi.ERR_INVALID and not out and 'ABI version mismatch' in msg


@pytest.mark.parametrize('field', ['vlosMu', 'wavelength'])
def test_refuses_missing_arrays(hip_lib, field):
    desc = small_prd_problem().descriptor()
    setattr(desc, field, None)
    st, out, msg = call_build(hip_lib, desc)
    assert st == abi.ERR_INVALID and not out and ('no ' + field[:4]) in msg, msg


def test_refuses_a_prd_line_with_one_wavelength(hip_lib):
    prob = small_prd_problem()
    desc = prob.descriptor()
    ia, kr = next((ia, kr) for ia, a in enumerate(prob.atoms) for kr, t in enumerate(a.trans) if t.rhoPrd is not None)
    desc.atoms[ia].trans[kr].Nred = desc.atoms[ia].trans[kr].Nblue + 1
    st, out, msg = call_build(hip_lib, desc)
    assert st == abi.ERR_INVALID and not out and 'fewer than 2 wavelengths' in msg


def test_refuses_2d(hip_lib):
    desc = small_prd_problem().descriptor()
    grid = abi.lwhip_grid2d()   # (refused for being there, before anything of it is read)
    desc.grid2d = C.cast(C.pointer(grid), C.c_void_p)
    st, out, msg = call_build(hip_lib, desc)
    assert st == abi.ERR_UNSUPPORTED and not out and '1D contexts only' in msg


def test_no_prd_line_is_ok_and_null(hip_lib):
    """The reference returns early and stays plain PRD: LWHIP_OK, no tables, with or without a device."""
    prob = plain_problem()
    desc = prob.descriptor()
    st, out, _ = call_build(hip_lib, desc)
    assert st == abi.OK and not out
    st, out, _ = call_build(hip_lib, desc, includeDetailed=1)
    assert st == abi.OK and not out
    from lightweaver_amd.hprd import build_hprd
    assert build_hprd(prob) is None


def test_no_cpu_fallback_without_gpu(hip_lib):
    if hip_lib.lwhip_device_count() > 0:
        pytest.skip('a GPU is present')
    prob = small_prd_problem()
    st, out, msg = call_build(hip_lib, prob.descriptor())
    assert st == abi.ERR_DEVICE and not out and 'no HIP device' in msg
    from lightweaver_amd.hprd import build_hprd
    with pytest.raises(context.LwHipError, match='no HIP device'):
        build_hprd(prob)
    with pytest.raises(context.LwHipError, match='no HIP device'):
        context.Context(prob.copy(), hprd=True)


def test_free_null_is_a_no_op_and_foreign_tables_are_left_alone(hip_lib):
    hip_lib.lwhip_hprd_free(None)

    class Foreign(C.Structure):   # (what follows a foreign descriptor in memory is not the library's mark)
        _fields_ = [('h', abi.lwhip_hprd), ('after', C.c_uint64 * 4)]
    foreign = Foreign()
    foreign.h.NprdLambda = 7
    hip_lib.lwhip_hprd_free(C.pointer(foreign.h))
    assert foreign.h.NprdLambda == 7 and not any(foreign.after)


def test_abi_is_additive(hip_lib):
    assert hip_lib.lwhip_abi_version() == abi.ABI_VERSION == 4
    txt = open(HEADER).read()
    assert re.search(r'#define LWHIP_ABI_VERSION 4\b', txt)
    bound = {name: (res, args) for name, res, args in abi.SYMBOLS}
    for name in ('lwhip_hprd_build', 'lwhip_hprd_free'):
        assert re.search(r'\b%s\s*\(' % name, txt) and name in bound and hasattr(hip_lib, name)
    assert bound['lwhip_hprd_build'][0] is C.c_int and len(bound['lwhip_hprd_build'][1]) == 4
    assert bound['lwhip_hprd_free'][0] is None
