"""The 2D pipeline's parity matrix: every template instance its launchers can pick, asserted through Context.layout_2d()
(lwhip_layout_2d) and compared with the C oracle, which tests/test_fs2d.py ties bit for bit to the reference's core.

Every geometry is built by the library's own build_grid2d; nothing here needs oracle/_ref except the two narrow-grid
comparisons that say so.  Problems are small: `columns` of FAL-C resampled to 6 planes, H_6(0.1) (84 wavelengths), one
iteration and a stat_equil unless a case says otherwise.  Tolerances are those of tests/test_fs2d.py (I, Psi*, J, Rij, Rji
1e-9 relative, times it + 1 across iterations; Gamma 1e-8; populations 1e-8; depth data 1e-9 as in tests/test_deep_columns.py).

What layout_2d() reports for the cases of this file (MI355X, default environment):

  fs2d_scan_kernel<D, FULL>   Nx = 37 <1, false>   64 <1, true>    100 <2, false>  128 <2, true>   130 <4, false>
                              256 <4, true>   300 <8, false>  512 <8, true>   576 <16, false>  1024 <16, true>
                              (both routes: the context's packed records + fs2d_longchar_kernel, and the primitive's whole
                              records with the long characteristics walked inside fs2d_coef_kernel<true>)
  gather2d_kernel<MAXL>       <2> H_6, H + Ca II      <4> blended_atoms(2)      <8> the three Ca II of blended_atoms(3)
  rates2d_kernel<MAXL, MAXM, MAXP>, by atom set -- (maxL, maxM, maxP) are the most lines / mixed / pure continua at one
  wavelength, counted on the host by slot_counts() below:
      Ca II alone         (2, 0, 5)   -> <2, 1, 5>
      H_6                 (1, 1, 3)   -> <2, 1, 5>
      H + Ca II           (2, 1, 7)   -> <2, 4, 8>   (more than five pure continua below 91 nm: H's and Ca II's)
      H + D_6             (2, 2, 6)   -> <2, 4, 8>
      blended_atoms(2)    (4, 1, 12)  -> <4, 4, 8>   (12 pure continua > MAXP = 8: four go straight to memory)
      blended_atoms(3)[1:]  (6, 0, 15)  -> <8, 4, 8> (its three Ca II without hydrogen; 15 > 8 again)
      blended_atoms(3)    (6, 1, 17)  -> refused by lwhip_create: its 17 continua at 70 .. 91 nm need 65 continuum rows
                                         (continuum_rows() below) and the rates kernel's LDS block holds 64
  Not reachable with whole harness atoms:
      <2, 2, 5>  needs two mixed continua at one wavelength (maxM = 2) with at most five pure ones anywhere.  One harness atom
                 never has two: a line couples only the continuum of its own upper or lower level that is active there (H_6:
                 one at Ly alpha, H alpha, H beta, Pa beta; Ca II: its continua end at 142 nm, its lines start at 393 nm).  Two
                 mixed continua therefore need two atoms with overlapping lines (H + D_6), and those have six pure continua at
                 570 .. 820 nm (levels 3, 4, 5 of each): maxP <= 5 fails.
      <4, 2, 5>  needs three or four lines at one wavelength.  No harness atom has three of its own lines at one wavelength, so
                 that takes lines of two atoms or more, whose continua together exceed five at one wavelength (two Ca II: ten
                 at 70 .. 104 nm; H + D_6: six): maxP <= 5 fails again.
  Not reachable either: nSlot = min(.., MAXSLOT) actually clamping.  MAXSLOT is at least 14 (<2, 4, 8>), and more than 14
  transitions at one wavelength of harness atoms means at least three atoms' continua there (an atom has at most five or six at
  one wavelength); <2, 4, 8> allows two lines, which three atoms exceed (their continua come with overlapping lines only for
  copies of one atom), <4, 4, 8> (MAXSLOT 16) needs 17 slots = 65 rows, and <8, 4, 8> (20) needs 21: both beyond the 64 rows.
  What does run is the branch next to it, pure continua beyond MAXP whose sums go straight to memory.
"""
import functools
import os
import time

import numpy as np
import pytest

from helpers import gamma_err_scaled, rel_err
from lightweaver_amd import _abi as abi
from lightweaver_amd.grid2d import build_grid2d
from oracle import bindings
from test_fs2d import blended_atoms, fields, prd_problem_2d
from test_geom2d import same_table

HAVE_REF = os.path.exists(bindings.REF_LIB)
BCS = [(abi.BC_THERMALISED, abi.BC_ZERO), (abi.BC_ZERO, abi.BC_THERMALISED)]
SCAN = {37: (1, False), 64: (1, True), 100: (2, False), 128: (2, True), 130: (4, False), 256: (4, True), 300: (8, False),
        512: (8, True), 576: (16, False), 1024: (16, True)}


def spacing(Nx):
    return 60e3 if Nx <= 128 else 30e3


def columns(Nx, Nz=6, seed0=700):
    from lightweaver_amd.harness import models
    base = models.resample(models.falc82(), Nz)
    return [models.perturbed(base, seed=seed0 + j) for j in range(Nx)]        # every column its own seed


def problem(Nx, Nz=6, dx=None, atoms=None, Nmuz=2, seed0=700, storeDepthData=False):
    from lightweaver_amd.harness import models
    dx = spacing(Nx) if dx is None else dx
    p = models.build_problem_2d(columns(Nx, Nz, seed0), np.arange(Nx) * dx, atoms or [models.H_6(0.1)], Nmuz=Nmuz)
    if storeDepthData:
        p.storeDepthData = True
        p.depthChi, p.depthEta, p.depthI = (np.zeros((p.Nlambda, p.Nrays, 2, p.Nspace)) for _ in range(3))
    return p


def bare_grid(Nx, Nz=6, dx=None, Nmuz=2, bc=BCS[0], seed0=700):
    """The geometry of problem(Nx, Nz, dx) without its atoms (the primitive route needs no more)."""
    from lightweaver_amd.harness import models
    cols = columns(Nx, Nz, seed0)
    mux, muz, _ = models.rays_2d(Nmuz)
    T = np.stack([c.temperature for c in cols], axis=-1)
    return build_grid2d(np.arange(Nx) * (spacing(Nx) if dx is None else dx), cols[0].height, mux, muz, T, bc[0], bc[1])


def long_char_lengths(grid):
    return np.diff(grid.substepOff)


def slot_counts(prob):
    """Per wavelength: lines, mixed continua, pure continua -- counted on the host from the problem's transitions by the
    definition DESIGN.md gives (all atoms active): a continuum is mixed where an active line of its own atom shares a level
    with it, or where its atom has lines but is not one of the first two atoms with lines (no moment slot)."""
    out = np.zeros((prob.Nlambda, 3), dtype=int)
    for la in range(prob.Nlambda):
        lines, conts = [], []
        for ia, a in enumerate(prob.atoms):
            for t in a.trans:
                if t.Nblue <= la < t.Nred:
                    (lines if t.type == abi.LINE else conts).append((ia, t.i, t.j))
        withLines = []
        for ia, _, _ in lines:
            if ia not in withLines:
                withLines.append(ia)
        nMixed = 0
        for ia, i, j in conts:
            shares = any(la_ == ia and (li in (i, j) or lj in (i, j)) for la_, li, lj in lines)
            nMixed += shares or (ia in withLines and withLines.index(ia) >= 2)
        out[la] = (len(lines), nMixed, len(conts) - nMixed)
    return out


def continuum_rows(prob):
    """The most continuum rows one wavelength needs in the 2D rates kernel's LDS block (chi_c and eta_c, eta per
    atom, chi and U per level its continua touch, Vji per continuum); lwhip_create refuses more than 64."""
    best = 0
    for la in range(prob.Nlambda):
        conts = [(ia, t.i, t.j) for ia, a in enumerate(prob.atoms) for t in a.trans
                 if t.type != abi.LINE and t.Nblue <= la < t.Nred]
        if conts:
            levels = {(ia, l) for ia, i, j in conts for l in (i, j)}
            best = max(best, 2 + len({ia for ia, _, _ in conts}) + 2 * len(levels) + len(conts))
    return best


def check_iteration(prob, q, it, up=None, dJ=None, what=''):
    errs = {'J': rel_err(prob.J, q.J), 'I': rel_err(prob.I, q.I)}
    for ia, (a, b) in enumerate(zip(prob.atoms, q.atoms)):
        errs[f'Gamma{ia}'] = rel_err(a.Gamma, b.Gamma)
        errs[f'Rij{ia}'] = max(rel_err(ta.Rij, tb.Rij) for ta, tb in zip(a.trans, b.trans))
        errs[f'Rji{ia}'] = max(rel_err(ta.Rji, tb.Rji) for ta, tb in zip(a.trans, b.trans))
    print(what, 'iteration', it, {k: f'{v:.2e}' for k, v in errs.items()})
    if up is not None:
        assert up.dJMax == pytest.approx(dJ, rel=1e-9)
    for k, v in errs.items():
        assert v <= (1e-8 if k.startswith('Gamma') else 1e-9 * (it + 1)), (what, it, k, v)


def iterate_against_oracle(prob, nIter=1, what=''):
    """nIter x (formal_sol_gamma_matrices, stat_equil) on the device and in the oracle, compared after every call; returns
    the context's layout_2d()."""
    from lightweaver_amd.context import Context
    q = prob.copy()
    orc = bindings.OracleContext(q)
    t0 = time.perf_counter()
    with Context(prob) as ctx:
        assert ctx.sweep_kind() == '2d'
        lay = ctx.layout_2d()
        for it in range(nIter):
            up = ctx.formal_sol_gamma_matrices()
            q.gamma_prefill()
            dJ, _ = orc.formal_sol_gamma_matrices()
            check_iteration(prob, q, it, up, dJ, what)
            ctx.stat_equil()
            assert orc.stat_equil() == 0
            en = max(rel_err(a.n, b.n) for a, b in zip(prob.atoms, q.atoms))
            print(what, 'populations', f'{en:.2e}')
            assert en <= 1e-8, (what, it, en)
    print(what, 'layout', lay, f'{time.perf_counter() - t0:.2f} s')
    return lay


def primitive_against_oracle(grid, seed=5, what=''):
    """lwhip_formal_solver_2d on every direction of the grid in one call, against the oracle's piecewise_besser_2d."""
    from lightweaver_amd.grid2d import formal_solver_2d
    chi, S = fields(grid, seed)
    rays = np.arange(2 * grid.Nrays, dtype=np.int32)
    I, P = formal_solver_2d(grid, 500.0, rays, np.broadcast_to(chi, (rays.size,) + chi.shape),
                            np.broadcast_to(S, (rays.size,) + S.shape))
    worst = 0.0
    for p, ray in enumerate(rays):
        Io, Po = bindings.oracle_2d_besser(grid, int(ray >> 1), int(ray & 1), 500.0, chi, S)
        eI, eP = rel_err(I[p], Io), rel_err(P[p], Po)
        worst = max(worst, eI, eP)
        assert eI <= 1e-9 and eP <= 1e-9, (what, int(ray), eI, eP)
    print(what, 'primitive', f'{worst:.2e}')


# ---- scan instances ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('Nx', sorted(SCAN))
def test_scan_instances_context_route(gpu, Nx):
    """fs2d_scan_kernel<D, FULL> behind a context: packed records, fs2d_longchar_kernel, fs2d_coef_kernel<false>."""
    prob = problem(Nx)
    g = prob.grid2d
    n = long_char_lengths(g)
    assert n.size > 0 and n.min() >= 2 and set(np.unique(g.uw['axis'])) == {0, 1, 2}
    lay = iterate_against_oracle(prob, what=f'Nx={Nx}')
    assert lay['scan'] == SCAN[Nx] and lay['packed'] and lay['NlongChar'] == n.size
    assert lay['gather'] == 2 and lay['rates'] == (2, 1, 5) and lay['batch2d'] == prob.Nlambda


@pytest.mark.gpu
@pytest.mark.parametrize('Nx', sorted(SCAN))
def test_scan_instances_primitive_route(gpu, Nx):
    """The same widths through lwhip_formal_solver_2d: whole records, long characteristics walked inline (it launches by the
    rule layout_2d reports for a context of this width -- fs2d_scan_instance(Nx) -- asserted in the context route)."""
    grid = bare_grid(Nx)
    assert long_char_lengths(grid).size > 0
    primitive_against_oracle(grid, what=f'Nx={Nx}')


@pytest.mark.gpu
@pytest.mark.parametrize('Nx', [128, 100])
def test_primitive_other_z_boundaries(gpu, Nx):
    """Both z-boundary pairs at one FULL and one ragged width (the default pair runs in the test above)."""
    for bc in BCS:
        primitive_against_oracle(bare_grid(Nx, bc=bc), what=f'Nx={Nx} bc={bc}')


# ---- storeDepthData, and both routes on one table ------------------------------------------------------------------------
def _depth_errs(p, q):
    return {name: rel_err(getattr(p, name), getattr(q, name)) for name in ('depthChi', 'depthEta', 'depthI')}


@pytest.mark.gpu
def test_depth_data_and_both_routes_on_one_table(gpu):
    """storeDepthData on a 2D context: the a.storeDepth branches of gather2d_kernel and rates2d_kernel against the oracle;
    formal_sol leaves the depth data alone, as the reference's does (intensity_core_opt<.., StoreDepthData = false>).  Then
    the primitive on this context's own table and opacities: the whole-record route with inline long characteristics gives
    the intensities the packed route with fs2d_longchar_kernel gave."""
    from lightweaver_amd.context import Context
    from lightweaver_amd.grid2d import formal_solver_2d
    prob = problem(10, storeDepthData=True)
    g = prob.grid2d
    Nx = g.Nx
    assert long_char_lengths(g).size > 0
    Jdag = prob.J.copy()
    q = prob.copy()
    orc = bindings.OracleContext(q)
    with Context(prob) as ctx:
        lay = ctx.layout_2d()
        assert lay['packed'] and lay['NlongChar'] > 0
        up = ctx.formal_sol_gamma_matrices()
        q.gamma_prefill()
        dJ, _ = orc.formal_sol_gamma_matrices()
        check_iteration(prob, q, 0, up, dJ, 'depth')
        e = _depth_errs(prob, q)
        print('depth data after the iteration', e)
        assert q.depthI.min() >= 0.0 and q.depthChi.min() > 0.0
        assert max(e.values()) <= 1e-9, e
        # Spectrum::I is the top plane of the up-going rays
        assert np.array_equal(prob.depthI[:, :, 1, :Nx], prob.I)
        after = {k: getattr(prob, k).copy() for k in ('depthChi', 'depthEta', 'depthI')}
        for upOnly in (False, True):
            prob.I[:] = -1.0
            ctx.formal_sol(upOnly=upOnly)
            ctx.download(abi.DEPTHDATA)
            orc.formal_sol(upOnly=upOnly)
            eI = rel_err(prob.I, q.I)
            e = _depth_errs(prob, q)
            print('formal_sol upOnly =', upOnly, 'I', eI, e)
            assert eI <= 1e-9 and max(e.values()) <= 1e-9, (upOnly, eI, e)
            # (J moved in the iteration, so this formal solution's I is not the stored one: storing it would show)
            assert rel_err(prob.I, after['depthI'][:, :, 1, :Nx]) > 1e-6
            for k, v in after.items():
                assert np.array_equal(getattr(prob, k)[:, :, 0], v[:, :, 0]), (upOnly, k)     # down-going rows untouched
    # the primitive on the table of this context, chi and S of one line-core and one continuum wavelength as the iteration
    # formed them (the oracle's depth data, S = (eta + sca Jdag) / chi)
    for la in (int(np.argmax(q.depthChi[:, 0, 1, 0])), prob.Nlambda - 1):
        chi = q.depthChi[la].reshape(2 * g.Nrays, g.Nz, Nx)
        S = ((q.depthEta[la] + (prob.bgSca[la] * Jdag[la])[None, None, :]) / q.depthChi[la]).reshape(chi.shape)
        rays = np.arange(2 * g.Nrays, dtype=np.int32)
        I, _ = formal_solver_2d(g, float(prob.wavelength[la]), rays, chi, S)
        want = q.depthI[la].reshape(chi.shape)
        have = after['depthI'][la].reshape(chi.shape)
        ePrim, eCtx = rel_err(I, want), rel_err(have, want)
        print('la', la, 'primitive vs oracle', ePrim, 'context vs oracle', eCtx)
        assert ePrim <= 1e-9 and eCtx <= 1e-9
        # the two routes' top planes: each within 1e-9 of the oracle, so within 2e-9 of each other
        assert rel_err(I[1::2, 0, :], have[1::2, 0, :]) <= 2e-9


# ---- plane and column edges ----------------------------------------------------------------------------------------------
EDGES = [(2, 2), (3, 2), (2, 3), (4, 3), (3, 4)]


def edge_case(Nx, Nz):
    return dict(Nx=Nx, Nz=Nz, dx=3e6, Nmuz=1 if (Nx, Nz) == (2, 2) else 2)


@pytest.mark.gpu
@pytest.mark.parametrize('Nx,Nz', EDGES)
def test_plane_and_column_edges(gpu, Nx, Nz):
    """Nz = 2 and 3: the scan's two-plane prefetch has nothing (or one plane) to fetch ahead; Nx = 2 and 3: one wavefront
    holds 62 idle lanes.  Both routes."""
    kw = edge_case(Nx, Nz)
    prob = problem(**kw)
    nLc = long_char_lengths(prob.grid2d).size
    assert 0 < nLc <= 12
    lay = iterate_against_oracle(prob, what=f'{Nx}x{Nz}')
    assert lay['scan'] == (1, False) and lay['NlongChar'] == nLc
    primitive_against_oracle(bare_grid(**kw), what=f'{Nx}x{Nz}')


# ---- ray counts ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('Nmuz', [1, 3, 16])
def test_ray_counts(gpu, Nmuz):
    """2, 6 and 32 rays (32: the most rates2d_kernel's ray table in LDS holds, 64 directions)."""
    kw = dict(Nx=6, Nz=8, dx=3e7, Nmuz=Nmuz) if Nmuz == 16 else dict(Nx=6, Nmuz=Nmuz)
    prob = problem(**kw)
    assert prob.Nrays == 2 * Nmuz
    lay = iterate_against_oracle(prob, what=f'Nmuz={Nmuz}')
    assert lay['scan'] == (1, False) and lay['NlongChar'] == long_char_lengths(prob.grid2d).size
    primitive_against_oracle(bare_grid(**kw), what=f'Nmuz={Nmuz}')


def test_more_than_32_rays_are_refused(hip_lib):
    """34 rays would overrun rates2d_kernel's LDS ray table: lwhip_create refuses before anything touches a device (the
    validation comes before the device is even looked for, so this runs anywhere)."""
    from lightweaver_amd.context import Context, LwHipError
    prob = problem(Nx=6, Nz=8, dx=3e7, Nmuz=17)
    assert prob.Nrays == 34
    with pytest.raises(LwHipError, match=rf'\({abi.ERR_UNSUPPORTED}\).*rates2d_kernel'):
        Context(prob)


@pytest.mark.gpu
def test_layout_2d_refuses_a_1d_context(gpu):
    from lightweaver_amd.context import Context, LwHipError
    from lightweaver_amd.harness import models
    with Context(models.falc_h(Nrays=3, lineScale=0.1)) as ctx:
        assert ctx.sweep_kind() != '2d'
        with pytest.raises(LwHipError, match=rf'\({abi.ERR_UNSUPPORTED}\).*not a 2D context'):
            ctx.layout_2d()


# ---- blends: the MAXL = 8 instances, pure continua beyond MAXP ---------------------------------------------------------------
def atom_sets():
    from lightweaver_amd.harness import models
    ls = 0.1
    return {'Ca': ([models.CaII_6(ls)], 2, (2, 1, 5)),
            'H': ([models.H_6(ls)], 2, (2, 1, 5)),
            'H+Ca': ([models.H_6(ls), models.CaII_6(ls)], 2, (2, 4, 8)),
            'H+D': ([models.H_6(ls), models.D_6(ls)], 2, (2, 4, 8)),
            'blend2': (blended_atoms(2, ls), 4, (4, 4, 8)),
            'Ca3': (blended_atoms(3, ls)[1:], 8, (8, 4, 8))}


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['Ca', 'H+Ca', 'H+D', 'blend2', 'Ca3'])
def test_rates_and_gather_instances(gpu, name):
    """Every reachable rates2d_kernel / gather2d_kernel instance (the module docstring's table; 'H' runs in every other
    test of this file).  The blends have more pure continua at one wavelength than MAXP = 8: the sums of those beyond MAXP
    go straight to memory.  Two iterations for them, as test_hip_2d_overlapping_lines does."""
    atoms, gather, rates = atom_sets()[name]
    prob = problem(6, atoms=atoms, seed0=300)
    n = slot_counts(prob)
    print(name, 'most lines / mixed / pure continua at one wavelength', n.max(axis=0), 'Nlambda', prob.Nlambda)
    blend = name in ('blend2', 'Ca3')
    assert continuum_rows(prob) <= 64
    lay = iterate_against_oracle(prob, nIter=2 if blend else 1, what=name)
    assert lay['gather'] == gather and lay['rates'] == rates
    assert n[:, 0].max() <= gather and n[:, 1].max() <= rates[1]
    if blend:
        assert n[:, 2].max() > rates[2]                                   # pure continua beyond MAXP
    if name == 'Ca3':
        assert n[:, 0].max() == 6


@pytest.mark.gpu
def test_blended_atoms_3_with_hydrogen_is_refused(gpu):
    """H + three Ca II: 17 continua at one wavelength need 65 continuum rows, one more than rates2d_kernel's LDS block
    holds; lwhip_create says so (the tables are built after the device is found, hence a GPU test)."""
    from lightweaver_amd.context import Context, LwHipError
    prob = problem(6, atoms=blended_atoms(3, 0.1), seed0=300)
    assert continuum_rows(prob) == 65 and slot_counts(prob)[:, 2].max() == 17
    with pytest.raises(LwHipError, match=rf'\({abi.ERR_UNSUPPORTED}\).*continuum rows'):
        Context(prob)


# ---- wavelength batches and groups -----------------------------------------------------------------------------------------
def _run(prob, nIter=1, prd=False):
    from lightweaver_amd.context import Context
    ups = []
    with Context(prob) as ctx:
        lay = ctx.layout_2d()
        for it in range(nIter):
            ctx.formal_sol_gamma_matrices()
            if prd:
                ups.append(ctx.prd_redistribute(3, 1e-2))
            else:
                ctx.stat_equil()
    return lay, ups


def _same_as_unbatched(p, ref, what):
    """The bounds of test_hip_2d_device_resident_and_batches (J 1e-11, n 1e-10); I and the rates, sums of terms of one sign,
    at J's bound; Gamma, whose terms cancel, at that bound on the scale of its terms (helpers.gamma_term_scale)."""
    errs = {'J': rel_err(p.J, ref.J), 'I': rel_err(p.I, ref.I)}
    for ia, (a, b) in enumerate(zip(p.atoms, ref.atoms)):
        errs[f'Gamma{ia}'] = gamma_err_scaled(a.Gamma, b)
        errs[f'R{ia}'] = max(max(rel_err(ta.Rij, tb.Rij), rel_err(ta.Rji, tb.Rji)) for ta, tb in zip(a.trans, b.trans))
    en = max(rel_err(a.n, b.n) for a, b in zip(p.atoms, ref.atoms))
    print(what, 'against the unbatched run', {k: f'{v:.2e}' for k, v in errs.items()}, f'n {en:.2e}')
    assert max(errs.values()) <= 1e-11 and en <= 1e-10, (what, errs, en)


@functools.lru_cache(maxsize=None)
def _batch_reference():
    """One 10-column problem: the unbatched device run and the oracle's iteration, shared by the batch cases (read only)."""
    base = problem(10, seed0=900)
    ref = base.copy()
    lay, _ = _run(ref)
    q = base.copy()
    orc = bindings.OracleContext(q)
    q.gamma_prefill()
    orc.formal_sol_gamma_matrices()
    assert orc.stat_equil() == 0
    return base, ref, q, lay


@pytest.mark.gpu
@pytest.mark.parametrize('batch', [1, 5, 83, 84])
def test_wavelength_batches_and_groups(gpu, monkeypatch, batch):
    """LWHIP_BATCH2D: 5 leaves a last batch of 4 wavelengths for 5 groups (an empty [bLo, bHi) group), 83 a last batch of
    one wavelength for 16 groups."""
    base, ref, q, layRef = _batch_reference()
    Nla = base.Nlambda
    assert Nla == 84 and layRef['batch2d'] == Nla and layRef['groups2d'] == 16
    check_iteration(ref, q, 0, what='unbatched')
    monkeypatch.setenv('LWHIP_BATCH2D', str(batch))
    p = base.copy()
    lay, _ = _run(p)
    print('batch', batch, lay)
    assert lay['batch2d'] == batch and lay['groups2d'] == min(16, batch)
    last = Nla % batch or batch
    assert {1: last == 1, 5: last == 4 and last < lay['groups2d'], 83: last == 1 and last < lay['groups2d'], 84: last == 84}[batch]
    _same_as_unbatched(p, ref, f'batch {batch}')
    check_iteration(p, q, 0, what=f'batch {batch}')
    assert max(rel_err(a.n, b.n) for a, b in zip(p.atoms, q.atoms)) <= 1e-8


def prd_runs(prob):
    """[lo, hi) runs of consecutive wavelengths that hold a PRD line (what the PRD rates pass, mode 3, visits)."""
    has = np.zeros(prob.Nlambda, dtype=bool)
    for a in prob.atoms:
        for t in a.trans:
            if t.type == abi.LINE and t.rhoPrd is not None:
                has[t.Nblue:t.Nred] = True
    edges = np.flatnonzero(np.diff(np.concatenate([[0], has.astype(int), [0]])))
    return list(zip(edges[::2], edges[1::2]))


@pytest.mark.gpu
def test_prd_rates_pass_across_batch_ends(gpu, monkeypatch):
    """prd_problem_2d with a batch shorter than its run of PRD wavelengths: the rates pass (mode 3) starts its batches at
    the run, the iteration at multiples of the batch; both cut the run.
    No population update between the iteration and the redistribution.  With one, the batched and the unbatched run
    differed by 2.4e-10 in n, 1.6e-11 in J and 1.2e-11 in the PRD lines' rates (bounds 1e-10 and 1e-11) although their J
    and I of the iteration were bit-equal and their Gamma agreed to 9e-16 of its terms: the rate matrices of this problem
    turn a change of 1e-15 of Gamma's terms into 1e-10 (H, depth 50) to 4e-10 (Ca II, depth 38) of n -- measured with the
    oracle's stat_equil on a perturbed Gamma --, and rho and J inherit it.  That is the inputs' conditioning, not the
    batches: the populations stay an input here, so that what is compared is what the batches compute."""
    base = prd_problem_2d()
    runs = prd_runs(base)
    lo, hi = max(runs, key=lambda r: r[1] - r[0])
    batch = int(hi - lo) // 2 + 1
    while lo % batch == 0:                   # the iteration's batch ends must not coincide with the run's start
        batch += 1
    assert lo + batch < hi                                       # mode 3: a batch ends inside the run
    assert (lo // batch + 1) * batch < hi and lo % batch != 0    # mode 0: so does one of the iteration's
    print('PRD runs', runs, 'batch', batch, 'of', base.Nlambda)
    ref = base.copy()
    layRef, upRef = _run(ref, prd=True)
    assert layRef['batch2d'] == base.Nlambda
    q = base.copy()
    orc = bindings.OracleContext(q)
    q.gamma_prefill()
    orc.formal_sol_gamma_matrices()
    ro = orc.redistribute_prd(3, 1e-2)
    monkeypatch.setenv('LWHIP_BATCH2D', str(batch))
    p = base.copy()
    lay, up = _run(p, prd=True)
    assert lay['batch2d'] == batch
    _same_as_unbatched(p, ref, f'PRD, batch {batch}')
    for t, u in zip(p.atoms[1].trans, ref.atoms[1].trans):
        if t.rhoPrd is not None:
            assert rel_err(t.rhoPrd, u.rhoPrd) <= 1e-11
    for r, w in ((upRef[0], 'unbatched'), (up[0], f'batch {batch}')):
        # the bounds of test_hip_2d_prd_matches_oracle, first iteration
        assert r.NprdSubIter == ro['NprdSubIter']
        print(w, 'dRho', rel_err(r.dRho, ro['dRho']), 'dJPrdMax', rel_err(r.dJPrdMax, ro['dJPrdMax']))
        assert rel_err(r.dRho, ro['dRho']) <= 1e-5 and rel_err(r.dJPrdMax, ro['dJPrdMax']) <= 1e-7
    for pp, w in ((ref, 'unbatched'), (p, f'batch {batch}')):
        errs = [rel_err(pp.J, q.J)]
        for a, b in zip(pp.atoms, q.atoms):
            for t, u in zip(a.trans, b.trans):
                if t.rhoPrd is not None:
                    errs.append(rel_err(t.rhoPrd, u.rhoPrd))
                errs += [rel_err(t.Rij, u.Rij), rel_err(t.Rji, u.Rji)]
        print(w, 'against the oracle', f'{max(errs):.2e}')
        assert max(errs) <= 1e-8, (w, errs)


# ---- narrow periodic grids: a shallow ray wraps round the domain many times ---------------------------------------------------
NARROW = [(3, 2, 2), (3, 2, 16), (6, 8, 2), (6, 8, 16)]        # Nx, Nz, Nmuz; 60 km columns


def narrow_inputs(Nx, Nz, Nmuz):
    from lightweaver_amd.harness import models
    cols = columns(Nx, Nz)
    mux, muz, _ = models.rays_2d(Nmuz)
    return np.arange(Nx) * 60e3, cols[0].height, mux, muz, np.stack([c.temperature for c in cols], axis=-1)


@pytest.mark.parametrize('Nx,Nz,Nmuz', NARROW)
def test_narrow_grids_build(hip_lib, Nx, Nz, Nmuz):
    """Grids the builder's former cap of 4 (Nx + Nz) + 16 sub-steps refused: they build, every long characteristic ends on
    a z plane (what the device's pass 1 relies on), and no walk is longer than the bound the builder derives."""
    from lightweaver_amd.context import LwHipError
    x, z, mux, muz, T = narrow_inputs(Nx, Nz, Nmuz)
    g = build_grid2d(x, z, mux, muz, T)
    n = long_char_lengths(g)
    assert n.size > 0 and n.min() >= 2
    assert np.all(g.substeps['axis'][g.substepOff[:-1]] != abi.AXIS_Z)
    assert n.max() > 4 * (Nx + Nz) + 16 + 1 or (Nx, Nz, Nmuz) == (6, 8, 2)     # the former cap really was in the way
    bound = np.ceil(np.abs(np.diff(z)).max() * np.abs(mux / muz).max() / 60e3) + 8 + 1
    assert n.max() <= bound
    with pytest.raises(LwHipError, match='muz = 0'):
        build_grid2d(x, z, np.append(mux, 1.0), np.append(muz, 0.0), T)         # a ray along x is still refused


@pytest.mark.skipif(not HAVE_REF, reason='oracle/_ref not built')
@pytest.mark.parametrize('Nx,Nz,Nmuz', NARROW)
def test_narrow_grids_match_reference(hip_lib, Nx, Nz, Nmuz):
    x, z, mux, muz, T = narrow_inputs(Nx, Nz, Nmuz)
    ref = bindings.Ref2d(x, z, mux, muz, T)
    grid = ref.grid()
    same_table(build_grid2d(x, z, mux, muz, T), grid)
    chi, S = fields(grid, 1)
    for mu in range(grid.Nrays):
        for toObs in (0, 1):
            Ir, Pr = ref.besser(mu, toObs, 500.0, chi, S)
            Io, Po = bindings.oracle_2d_besser(grid, mu, toObs, 500.0, chi, S)
            np.testing.assert_array_equal(Io, Ir)
            np.testing.assert_array_equal(Po, Pr)


@pytest.mark.gpu
def test_narrow_grid_on_the_device(gpu):
    """3 columns x 2 planes at 60 km, four rays: both routes."""
    prob = problem(3, Nz=2, dx=60e3)
    n = long_char_lengths(prob.grid2d)
    assert n.max() > 4 * (3 + 2) + 16 + 1
    lay = iterate_against_oracle(prob, what='narrow')
    assert lay['NlongChar'] == n.size and lay['packed']
    primitive_against_oracle(bare_grid(3, Nz=2, dx=60e3), what='narrow')
