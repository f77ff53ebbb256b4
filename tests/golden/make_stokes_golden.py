"""Generate tests/golden/falc_stokes_small.npz and falc_stokes_matrix.npz by running the REAL Lightweaver core's
full-Stokes path.

Runs only where the reference sources exist (/root/reference/Source, or LW_REFERENCE_SOURCE): it compiles
tests/golden/stokes_driver.cpp (which builds on oracle/ref_driver.cpp) together with the reference's own sources, with the
flags of oracle/Makefile, into a temporary directory; no compiled file enters the tree.  The Zeeman components come from
the reference's lightweaver/zeeman.py, loaded by file path.

    python tests/golden/make_stokes_golden.py [small] [matrix]      (default: both)

falc_stokes_small.npz.  Problem: harness.zeeman.falc_h_ca_stokes() -- FAL-C, H_6 + CaII_6 at lineScale 0.2, 3 rays (the last one mu = 1), a
depth-varying B, gammaB, chiB; Ca II H, K and the IR triplet polarised.  The atmosphere and atoms are rebuilt from the
harness by the tests (the fixture holds a few of their arrays to check that); the field, the rays, the components and
the projections are stored.  Keys:
  in/B, in/gammaB, in/chiB, in/mux, in/muy, in/muz, in/wavelength, in/bgChi, in/J   inputs (the last three: rebuild check)
  in/alpha<i>, in/shift<i>, in/strength<i>   Zeeman components of polarised line i (lightweaver/zeeman.py)
  in/cosGamma, in/cos2chi, in/sin2chi        Atmosphere::update_projections
  in/J20                                     J20 dagger of the J20 variant
  prof/<name><i>                             phi, phiQ..psiV of line i, every DEPTH_STRIDE-th depth; prof/wphi<i>
  out/up/{I,Quv}                             formal_sol_full_stokes(updateJ=False, upOnly=True)
  out/j/{I,Quv,J,dJMax,dJMaxIdx}             updateJ=True, upOnly=False
  out/j20/{I,Quv,J,J20,dJMax,dJMaxIdx}       the same with ExtraParams "J20"

falc_stokes_matrix.npz.  The cases of tests/stokes_cases.py (velocities, 3 to 130 depth points, 1 to 7 rays, CALLABLE
and THERMALISED boundaries on either side, a PRD line's rho, strong / zero / edge-on fields, J20), each rebuilt by the tests
from stokes_cases.build.  Keys:
  in/alpha<i>, in/shift<i>, in/strength<i>   Zeeman components of polarised line i (the same lines in every case)
  in/<case>/muz, in/<case>/vlosMu            rebuild check; in/<case>/bcData, in/<case>/J20: wavelength row ROW of them
  prof/<case>/<name><i>                      moving82 and fastv: phi, phiQ..psiV of line i at every DEPTH_STRIDE-th depth, wphi
  out/<case>/<variant>/{I,Quv}               variants up (updateJ False, upOnly True), j (True, False) and, for two cases,
                                             all (False, False) and jup (True, True).  Quv is stored as zero at
                                             wavelengths without a polarised line: the core leaves it unspecified there
  out/<case>/<variant>/{J,dJMax,dJMaxIdx}    with updateJ; J (and J20 of case j20) at the depths stokes_cases.j_depths
"""
import ctypes as C
import importlib.util
import os
import subprocess
import sys
import tempfile
import types
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from lightweaver_amd import _abi as abi  # noqa: E402
from lightweaver_amd.harness import zeeman  # noqa: E402

REF = os.environ.get('LW_REFERENCE_SOURCE', '/root/reference/Source')
REF_PY = os.path.join(os.path.dirname(REF), 'lightweaver', 'zeeman.py')
OUT = os.path.join(HERE, 'falc_stokes_small.npz')
OUT_MATRIX = os.path.join(HERE, 'falc_stokes_matrix.npz')
DEPTH_STRIDE = 8


def build_driver(tmp):
    lib = os.path.join(tmp, 'libstokesref.so')
    cmd = ['g++', '-std=c++17', '-O2', '-fPIC', '-shared', '-Wno-sign-compare', '-DENKITS_BUILD_DLL', '-DLW_CORE_LIB',
           f'-I{REF}', f'-I{os.path.join(ROOT, "include")}', '-o', lib, os.path.join(HERE, 'stokes_driver.cpp'),
           os.path.join(REF, 'LightweaverAmalgamated.cpp'), os.path.join(REF, 'TaskScheduler.cpp'),
           '-ldl', '-lpthread', '-Wl,-Bsymbolic']
    subprocess.run(cmd, check=True)
    lib = C.CDLL(lib)
    lib.lwref_create.restype = C.c_void_p
    lib.lwref_create.argtypes = [C.POINTER(abi.lwhip_problem), C.c_char_p, C.c_int, C.c_char_p, C.c_int]
    lib.lwref_destroy.argtypes = [C.c_void_p]
    lib.lwrefs_stokes.argtypes = [C.c_void_p, C.POINTER(abi.lwhip_stokes)] + [abi.f64p] * 5 + [
        C.POINTER(C.c_void_p), C.c_char_p, C.c_int]
    lib.lwrefs_polarised_profiles.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_int]
    lib.lwrefs_full_stokes.argtypes = [C.c_void_p, C.c_int, C.c_int, abi.f64p, C.POINTER(abi.lwhip_iter_result),
                                       C.c_char_p, C.c_int]
    lib.lwrefs_free.argtypes = [C.c_void_p]
    return lib


def reference_components(prob):
    """compute_zeeman_components of the reference for every polarised line (LS coupling from the CaII_6 terms)."""
    spec = importlib.util.spec_from_file_location('lw_zeeman_ref', REF_PY)
    zr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(zr)
    out = []
    for L in prob.stokes.lines:
        t = prob.atoms[L.atom].trans[L.trans]
        lev = lambda i: types.SimpleNamespace(J=zeeman.CAII_TERMS[i][0], L=zeeman.CAII_TERMS[i][1],
                                              S=zeeman.CAII_TERMS[i][2], lsCoupling=True)
        line = types.SimpleNamespace(gLandeEff=None, iLevel=lev(t.i), jLevel=lev(t.j))
        z = zr.compute_zeeman_components(line)
        out.append((np.ascontiguousarray(z.alpha, dtype=np.int32), np.asarray(z.strength, dtype=np.float64),
                    np.asarray(z.shift, dtype=np.float64)))
    return out


def run_variant(lib, comps, updateJ, upOnly, J20=None, prob=None):
    prob = zeeman.falc_h_ca_stokes() if prob is None else prob
    for L, (al, st, sh) in zip(prob.stokes.lines, comps):
        L.alpha, L.strength, L.shift = al, st, sh
    st = prob.stokes
    desc = prob.descriptor()
    sdesc = prob.stokes_descriptor()
    err = C.create_string_buffer(512)
    h = lib.lwref_create(C.byref(desc), None, 1, err, 512)
    assert h, err.value
    extra = C.c_void_p()
    p = lambda a: a.ctypes.data_as(abi.f64p)
    assert lib.lwrefs_stokes(h, C.byref(sdesc), p(st.gammaB), p(st.chiB), p(st.mux), p(st.muy), p(st.vz),
                             C.byref(extra), err, 512) == 0, err.value
    assert lib.lwrefs_polarised_profiles(h, extra, err, 512) == 0, err.value
    res = abi.lwhip_iter_result()
    j20 = None if J20 is None else J20.copy()
    assert lib.lwrefs_full_stokes(h, int(updateJ), int(upOnly), None if j20 is None else p(j20), C.byref(res),
                                  err, 512) == 0, err.value
    lib.lwrefs_free(extra)
    lib.lwref_destroy(h)
    return prob, res, j20


def make_small():
    if not os.path.exists(os.path.join(REF, 'LightweaverAmalgamated.cpp')) or not os.path.exists(REF_PY):
        print(f'reference sources not present at {REF}: nothing generated')
        return
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        lib = build_driver(tmp)
        comps = reference_components(zeeman.falc_h_ca_stokes())
        prob, _, _ = run_variant(lib, comps, False, True)
        st = prob.stokes
        for key in ('B', 'gammaB', 'chiB', 'mux', 'muy', 'cosGamma', 'cos2chi', 'sin2chi'):
            out[f'in/{key}'] = getattr(st, key).copy()
        out['in/muz'] = prob.muz.copy()
        out['in/wavelength'] = prob.wavelength.copy()
        out['in/bgChi'] = prob.bgChi[:, ::DEPTH_STRIDE].copy()
        out['in/J'] = prob.J[:, ::DEPTH_STRIDE].copy()
        ks = slice(None, None, DEPTH_STRIDE)
        for i, (L, (al, sg, sh)) in enumerate(zip(st.lines, comps)):
            out[f'in/alpha{i}'], out[f'in/strength{i}'], out[f'in/shift{i}'] = al, sg, sh
            t = prob.atoms[L.atom].trans[L.trans]
            out[f'prof/phi{i}'] = t.phi[..., ks].copy()
            out[f'prof/wphi{i}'] = t.wphi.copy()
            for name in ('phiQ', 'phiU', 'phiV', 'psiQ', 'psiU', 'psiV'):
                out[f'prof/{name}{i}'] = getattr(L, name)[..., ks].copy()
        out['out/up/I'] = prob.I.copy()
        out['out/up/Quv'] = prob.Quv.copy()
        prob, res, _ = run_variant(lib, comps, True, False)
        for key, v in (('I', prob.I), ('Quv', prob.Quv), ('J', prob.J)):
            out[f'out/j/{key}'] = v.copy()
        out['out/j/dJMax'], out['out/j/dJMaxIdx'] = np.array(res.dJMax), np.array(res.dJMaxIdx)
        rng = np.random.default_rng(11)
        J20 = 0.05 * prob.J * (rng.random(prob.J.shape) - 0.5)
        out['in/J20'] = J20
        prob, res, j20 = run_variant(lib, comps, True, False, J20=J20)
        for key, v in (('I', prob.I), ('Quv', prob.Quv), ('J', prob.J), ('J20', j20)):
            out[f'out/j20/{key}'] = v.copy()
        out['out/j20/dJMax'], out['out/j20/dJMaxIdx'] = np.array(res.dJMax), np.array(res.dJMaxIdx)
    np.savez_compressed(OUT, **out)
    print(f'wrote {OUT}: {os.path.getsize(OUT)} bytes')


def make_matrix():
    if not os.path.exists(os.path.join(REF, 'LightweaverAmalgamated.cpp')) or not os.path.exists(REF_PY):
        print(f'reference sources not present at {REF}: nothing generated')
        return
    from tests import stokes_cases as sc
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        lib = build_driver(tmp)
        comps = reference_components(sc.build('n3'))
        for i, (al, sg, sh) in enumerate(comps):
            out[f'in/alpha{i}'], out[f'in/strength{i}'], out[f'in/shift{i}'] = al, sg, sh
        for case in sc.CASES:
            base = sc.build(case)
            out[f'in/{case}/muz'] = base.muz.copy()
            out[f'in/{case}/vlosMu'] = base.vlosMu.copy()
            for bc in (base.zLowerBc, base.zUpperBc):
                if bc.type == abi.BC_CALLABLE:
                    out[f'in/{case}/bcData'] = bc.bcData[sc.MATRIX_ROW].copy()
            J20 = base.stokes.J20
            if J20 is not None:
                out[f'in/{case}/J20'] = J20[sc.MATRIX_ROW].copy()
            pol = sc.polarised_mask(base, j20=J20 is not None)
            kd = sc.j_depths(base.Nspace)
            for variant in sc.variants(case):
                updateJ, upOnly = sc.VARIANTS[variant]
                prob, res, j20 = run_variant(lib, comps, updateJ, upOnly, J20=J20, prob=sc.build(case))
                key = f'out/{case}/{variant}'
                out[f'{key}/I'] = prob.I.copy()
                out[f'{key}/Quv'] = np.where(pol[None, :, None], prob.Quv, 0.0)
                if updateJ:
                    out[f'{key}/J'] = prob.J[:, kd].copy()
                    out[f'{key}/dJMax'], out[f'{key}/dJMaxIdx'] = np.array(res.dJMax), np.array(res.dJMaxIdx)
                    if j20 is not None:
                        out[f'{key}/J20'] = j20[:, kd].copy()
                if case in sc.PROFILE_CASES and variant == 'up':
                    ks = slice(None, None, sc.DEPTH_STRIDE)
                    for i, L in enumerate(prob.stokes.lines):
                        t = prob.atoms[L.atom].trans[L.trans]
                        out[f'prof/{case}/phi{i}'] = t.phi[..., ks].copy()
                        out[f'prof/{case}/wphi{i}'] = t.wphi.copy()
                        for name in sc.PROFILE_NAMES:
                            out[f'prof/{case}/{name}{i}'] = getattr(L, name)[..., ks].copy()
    np.savez_compressed(OUT_MATRIX, **out)
    print(f'wrote {OUT_MATRIX}: {os.path.getsize(OUT_MATRIX)} bytes')


def main(argv):
    what = argv or ['small', 'matrix']
    if 'small' in what:
        make_small()
    if 'matrix' in what:
        make_matrix()


if __name__ == '__main__':
    main(sys.argv[1:])
