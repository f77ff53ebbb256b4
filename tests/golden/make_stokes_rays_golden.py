"""Generate tests/golden/falc_stokes_rays.npz by running the REAL Lightweaver core on the problem that
LwContext.compute_rays(mus, stokes=True) (Source/LwMiddleLayer.pyx:3898-4002) hands to its second context.

Runs only where the reference sources exist (as make_stokes_golden.py, whose driver and Zeeman components it uses: the
driver is compiled into a temporary directory; no compiled file enters the tree).

    python tests/golden/make_stokes_rays_golden.py

For every entry of tests/stokes_rays_cases.entries() -- six cases of tests/stokes_cases.py seen along MUS = [1.0, 0.6, 0.2]
with the reference's 1D azimuth (mux = sqrt(1 - mu^2), muy = 0), and moving82 at mu = 0.6 with mux = 0, muy = 0.8 -- the
observer problem (model.observer_problem(stokes=True): the same state, rays muz = mus, vlosMu = mu (x) v_z, wmu = 0) goes
through Atmosphere::update_projections, Transition::compute_phi of every line, Transition::compute_polarised_profiles of the
polarised ones and formal_sol_full_stokes(updateJ = 0, upOnly = 1).  Keys:
  in/mus                                       MUS
  in/<key>/{mus,mux,muy}                       the directions of the entry
  in/<key>/{cosGamma,cos2chi,sin2chi}          [Nmu, Nspace] Atmosphere::update_projections of the new directions
  in/<key>/lowerBc                             (CALLABLE lower boundary) wavelength row MATRIX_ROW of the data passed
  out/<key>/I [Nlambda, Nmu], out/<key>/Quv [3, Nlambda, Nmu]   Quv stored as zero at wavelengths without a polarised line
"""
import ctypes as C
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import make_stokes_golden as msg  # noqa: E402
from lightweaver_amd import _abi as abi  # noqa: E402
from tests import stokes_cases as sc  # noqa: E402
from tests import stokes_rays_cases as src  # noqa: E402

OUT = os.path.join(HERE, 'falc_stokes_rays.npz')


def run_observer(lib, comps, prob):
    """The core's observer route on `prob` (an observer problem with Stokes data); fills prob.I and prob.Quv."""
    for L, (al, sg, sh) in zip(prob.stokes.lines, comps):
        L.alpha, L.strength, L.shift = al, sg, sh
    st = prob.stokes
    desc = prob.descriptor()
    sdesc = prob.stokes_descriptor()
    err = C.create_string_buffer(512)
    h = lib.lwref_create(C.byref(desc), None, 1, err, 512)
    assert h, err.value
    extra = C.c_void_p()
    p = lambda a: a.ctypes.data_as(abi.f64p)
    # (the projections are written into st.cosGamma / cos2chi / sin2chi by Atmosphere::update_projections)
    assert lib.lwrefs_stokes(h, C.byref(sdesc), p(st.gammaB), p(st.chiB), p(st.mux), p(st.muy), p(st.vz),
                             C.byref(extra), err, 512) == 0, err.value
    assert lib.lwref_compute_profiles(h) == 0
    assert lib.lwrefs_polarised_profiles(h, extra, err, 512) == 0, err.value
    res = abi.lwhip_iter_result()
    assert lib.lwrefs_full_stokes(h, 0, 1, None, C.byref(res), err, 512) == 0, err.value
    lib.lwrefs_free(extra)
    lib.lwref_destroy(h)


def main():
    if not os.path.exists(os.path.join(msg.REF, 'LightweaverAmalgamated.cpp')) or not os.path.exists(msg.REF_PY):
        print(f'reference sources not present at {msg.REF}: nothing generated')
        return
    out = {'in/mus': src.MUS.copy()}
    with tempfile.TemporaryDirectory() as tmp:
        lib = msg.build_driver(tmp)
        lib.lwref_compute_profiles.argtypes = [C.c_void_p]
        comps = msg.reference_components(sc.build('n3'))
        for key, case, mus, mux, muy in src.entries():
            base = sc.build(case)
            prob = src.observer(base, mus, mux, muy)
            run_observer(lib, comps, prob)
            st = prob.stokes
            out[f'in/{key}/mus'], out[f'in/{key}/mux'], out[f'in/{key}/muy'] = prob.muz.copy(), st.mux.copy(), st.muy.copy()
            for name in ('cosGamma', 'cos2chi', 'sin2chi'):
                out[f'in/{key}/{name}'] = getattr(st, name).copy()
            if prob.zLowerBc.type == abi.BC_CALLABLE:
                out[f'in/{key}/lowerBc'] = prob.zLowerBc.bcData[sc.MATRIX_ROW].copy()
            pol = sc.polarised_mask(base)
            out[f'out/{key}/I'] = prob.I.copy()
            out[f'out/{key}/Quv'] = np.where(pol[None, :, None], prob.Quv, 0.0)
    np.savez_compressed(OUT, **out)
    print(f'wrote {OUT}: {os.path.getsize(OUT)} bytes')


if __name__ == '__main__':
    main()
