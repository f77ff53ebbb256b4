"""Host-side data model at the `Context` array boundary.

These classes own the numpy buffers that Lightweaver's Cython layer owns in the reference
(LwAtmosphere / LwSpectrum / LwBackground / LwAtom / LwTransition,
Source/LwMiddleLayer.pyx:639-689,2724-2732,1571-1597,2389-2406,1804-1825) and flatten them into
the `lwhip_problem` descriptor of include/lwhip.h.  Shapes follow SURVEY.md Appendix C:
everything C-contiguous float64, depth `k` fastest.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

from . import _abi as abi


def _f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None and tuple(a.shape) != tuple(shape):
        raise ValueError(f'expected shape {tuple(shape)}, got {a.shape}')
    return a


def _ptr(a):
    if a is None:
        return C.cast(None, abi.f64p)
    return a.ctypes.data_as(abi.f64p)


@dataclass
class TransitionData:
    """One line or continuum (Transition, Source/LwTransition.hpp:21-69)."""
    type: int
    i: int
    j: int
    Nblue: int
    Nred: int
    lambda0: float
    wavelength: np.ndarray                 # [NlaT] = global grid[Nblue:Nred]
    Aji: float = 0.0
    Bji: float = 0.0
    Bij: float = 0.0
    dopplerWidth: float = 1.0
    alpha: Optional[np.ndarray] = None     # [NlaT] continua
    phi: Optional[np.ndarray] = None       # [NlaT, Nrays, 2, Nspace] lines
    wphi: Optional[np.ndarray] = None      # [Nspace] lines
    aDamp: Optional[np.ndarray] = None     # [Nspace] lines
    rhoPrd: Optional[np.ndarray] = None    # [NlaT, Nspace] PRD lines
    Qelast: Optional[np.ndarray] = None    # [Nspace] elastic collision rate (PRD lines)
    Rij: Optional[np.ndarray] = None       # [Nspace]
    Rji: Optional[np.ndarray] = None       # [Nspace]

    @property
    def Nlambda(self):
        return self.Nred - self.Nblue

    def wlambda(self):
        """Trapezoid weights of the transition's own grid, Transition::wlambda
        (Source/LwTransition.hpp:71-81)."""
        w = self.wavelength
        out = np.empty_like(w)
        out[0] = 0.5 * (w[1] - w[0])
        out[-1] = 0.5 * (w[-1] - w[-2])
        out[1:-1] = 0.5 * (w[2:] - w[:-2])
        return out * self.dopplerWidth


@dataclass
class AtomData:
    """One atom (Atom, Source/LwAtom.hpp:41-80)."""
    name: str
    Nlevel: int
    n: np.ndarray                          # [Nlevel, Nspace]
    nStar: np.ndarray                      # [Nlevel, Nspace]
    nTotal: np.ndarray                     # [Nspace]
    vBroad: np.ndarray                     # [Nspace]
    trans: List[TransitionData] = field(default_factory=list)
    detailed: bool = False
    Gamma: Optional[np.ndarray] = None     # [Nlevel, Nlevel, Nspace] (to, from, k)
    C: Optional[np.ndarray] = None         # [Nlevel, Nlevel, Nspace]


@dataclass
class Boundary:
    """AtmosphericBoundaryCondition (Source/LwAtmosphere.hpp:17-43) for one z face."""
    type: int = abi.BC_ZERO
    idxs: Optional[np.ndarray] = None      # [Nrays, 2] int32
    bcData: Optional[np.ndarray] = None    # [Nlambda, Nmu]


def update_projections(muz, mux, muy, gammaB, chiB):
    """cosGamma, cos2chi, sin2chi [Nrays, Nspace] of the field (gammaB, chiB) [Nspace] seen along each ray:
    Atmosphere::update_projections (Source/Atmosphere.cpp:47-82), with its exact branch for muz == 1."""
    muz, mux, muy = (np.asarray(v, dtype=np.float64) for v in (muz, mux, muy))
    gammaB, chiB = np.asarray(gammaB, dtype=np.float64), np.asarray(chiB, dtype=np.float64)
    Nr, Ns = muz.shape[0], gammaB.shape[0]
    # (the C library's sin / cos, element by element: numpy's vectorised ones may differ from them in the last bit)
    import math
    _cos = lambda x: np.array([math.cos(v) for v in x])
    _sin = lambda x: np.array([math.sin(v) for v in x])
    cosGamma, cos2chi, sin2chi = np.empty((Nr, Ns)), np.empty((Nr, Ns)), np.empty((Nr, Ns))
    for mu in range(Nr):
        if muz[mu] == 1.0:
            cosGamma[mu] = _cos(gammaB)
            cos2chi[mu] = _cos(2.0 * chiB)
            sin2chi[mu] = _sin(2.0 * chiB)
            continue
        cscTheta = 1.0 / np.sqrt(1.0 - muz[mu] ** 2)
        sinGamma = _sin(gammaB)
        bx = sinGamma * _cos(chiB)
        by = sinGamma * _sin(chiB)
        bz = _cos(gammaB)
        b3 = mux[mu] * bx + muy[mu] * by + muz[mu] * bz
        b1 = cscTheta * (bz - muz[mu] * b3)
        b2 = cscTheta * (muy[mu] * bx - mux[mu] * by)
        cosGamma[mu] = b3
        cos2chi[mu] = (b1 ** 2 - b2 ** 2) / (1.0 - b3 ** 2)
        sin2chi[mu] = 2.0 * b1 * b2 / (1.0 - b3 ** 2)
    return cosGamma, cos2chi, sin2chi


@dataclass
class StokesLine:
    """One Zeeman-polarised line: prob.atoms[atom].trans[trans] with its components (ZeemanComponents,
    Source/LwMisc.hpp:106-111) and its polarised profiles (Transition::phiQ..psiV, Source/LwTransition.hpp:44-51)."""
    atom: int
    trans: int
    alpha: np.ndarray                      # [Ncomp] int32: -1 sigma_b, 0 pi, 1 sigma_r
    shift: np.ndarray                      # [Ncomp] in Larmor units
    strength: np.ndarray                   # [Ncomp]
    phiQ: Optional[np.ndarray] = None      # [NlaT, Nrays, 2, Nspace] each
    phiU: Optional[np.ndarray] = None
    phiV: Optional[np.ndarray] = None
    psiQ: Optional[np.ndarray] = None
    psiU: Optional[np.ndarray] = None
    psiV: Optional[np.ndarray] = None

    PROFILES = ('phiQ', 'phiU', 'phiV', 'psiQ', 'psiU', 'psiV')


@dataclass
class StokesData:
    """The magnetic field and the polarised lines of a full-Stokes problem (Atmosphere B, gammaB, chiB, mux, muy;
    Source/LwAtmosphere.hpp:190-200).  `Problem.set_stokes` derives the projections."""
    B: np.ndarray                          # [Nspace] T
    gammaB: np.ndarray                     # [Nspace] inclination
    chiB: np.ndarray                       # [Nspace] azimuth
    mux: np.ndarray                        # [Nrays]
    muy: np.ndarray                        # [Nrays]
    lines: List[StokesLine] = field(default_factory=list)
    cosGamma: Optional[np.ndarray] = None  # [Nrays, Nspace]
    cos2chi: Optional[np.ndarray] = None
    sin2chi: Optional[np.ndarray] = None
    J20: Optional[np.ndarray] = None       # [Nlambda, Nspace] ExtraParams "J20", or None
    vz: Optional[np.ndarray] = None        # [Nspace] vertical velocity vlosMu was made from (Atmosphere::vz), or None


class Problem:
    """Everything `Context&` reaches on the hot path, as owned numpy arrays."""

    def __init__(self, height, temperature, muz, wmu, wavelength, bgChi, bgEta, bgSca,
                 atoms: List[AtomData], vlosMu=None, J=None,
                 formalSolver=abi.FS_BEZIER3_1D,
                 zLowerBc: Optional[Boundary] = None, zUpperBc: Optional[Boundary] = None,
                 storeDepthData=False, grid2d=None):
        # 2D (x-periodic) geometry: a lightweaver_amd.grid2d.Grid2d; Nspace = Nz * Nx, index k * Nx + j
        self.grid2d = grid2d
        self.height = _f64(height)
        self.Nspace = self.height.shape[0]
        self.temperature = _f64(temperature, (self.Nspace,))
        self.muz = _f64(muz)
        self.Nrays = self.muz.shape[0]
        self.wmu = _f64(wmu, (self.Nrays,))
        self.wavelength = _f64(wavelength)
        self.Nlambda = self.wavelength.shape[0]
        shp = (self.Nlambda, self.Nspace)
        self.bgChi = _f64(bgChi, shp)
        self.bgEta = _f64(bgEta, shp)
        self.bgSca = _f64(bgSca, shp)
        self.vlosMu = (_f64(vlosMu, (self.Nrays, self.Nspace)) if vlosMu is not None
                       else np.zeros((self.Nrays, self.Nspace)))
        self.J = _f64(J, shp) if J is not None else np.zeros(shp)
        self.I = (np.zeros((self.Nlambda, self.Nrays)) if grid2d is None
                  else np.zeros((self.Nlambda, self.Nrays, grid2d.Nx)))
        if grid2d is not None and grid2d.Nx * grid2d.Nz != self.Nspace:
            raise ValueError('2D problem: Nspace must equal Nz * Nx')
        self.formalSolver = int(formalSolver)
        self.zLowerBc = zLowerBc if zLowerBc is not None else Boundary(abi.BC_THERMALISED)
        self.zUpperBc = zUpperBc if zUpperBc is not None else Boundary(abi.BC_ZERO)
        self.storeDepthData = bool(storeDepthData)
        self.depthChi = self.depthEta = self.depthI = None
        if self.storeDepthData:
            dshape = (self.Nlambda, self.Nrays, 2, self.Nspace)
            self.depthChi = np.zeros(dshape)
            self.depthEta = np.zeros(dshape)
            self.depthI = np.zeros(dshape)
        # active atoms first, then detailed (include/lwhip.h: lwhip_problem.Natom)
        self.atoms = [a for a in atoms if not a.detailed] + [a for a in atoms if a.detailed]
        for a in self.atoms:
            self._normalise_atom(a)
        self._keepalive = None
        self.stokes: Optional[StokesData] = None
        self.Quv = None

    def set_stokes(self, stokes: Optional[StokesData]):
        """Attach (or drop) the full-Stokes data; computes the projections (update_projections) and allocates Quv
        [3, Nlambda, Nrays] and every missing polarised profile."""
        self.stokes = stokes
        if stokes is None:
            self.Quv = None
            return
        Ns, Nr = self.Nspace, self.Nrays
        stokes.B = _f64(stokes.B, (Ns,))
        stokes.gammaB = _f64(stokes.gammaB, (Ns,))
        stokes.chiB = _f64(stokes.chiB, (Ns,))
        stokes.mux = _f64(stokes.mux, (Nr,))
        stokes.muy = _f64(stokes.muy, (Nr,))
        stokes.cosGamma, stokes.cos2chi, stokes.sin2chi = update_projections(
            self.muz, stokes.mux, stokes.muy, stokes.gammaB, stokes.chiB)
        if stokes.J20 is not None:
            stokes.J20 = _f64(stokes.J20, (self.Nlambda, Ns))
        for L in stokes.lines:
            t = self.atoms[L.atom].trans[L.trans]
            if t.type != abi.LINE:
                raise ValueError('a polarised transition must be a line')
            L.alpha = np.ascontiguousarray(L.alpha, dtype=np.int32)
            L.shift = _f64(L.shift, L.alpha.shape)
            L.strength = _f64(L.strength, L.alpha.shape)
            for name in StokesLine.PROFILES:
                a = getattr(L, name)
                setattr(L, name, _f64(a, t.phi.shape) if a is not None else np.zeros(t.phi.shape))
        self.Quv = np.zeros((3, self.Nlambda, Nr))

    def stokes_descriptor(self):
        """The lwhip_stokes descriptor of `self.stokes` (borrows its arrays; keep the Problem alive)."""
        st = self.stokes
        lines = (abi.lwhip_stokes_line * max(len(st.lines), 1))()
        for i, L in enumerate(st.lines):
            cl = abi.raw_view(lines[i])
            cl.atom, cl.trans, cl.Ncomp = int(L.atom), int(L.trans), int(L.alpha.shape[0])
            cl.alpha, cl.shift, cl.strength = abi.addr(L.alpha), abi.addr(L.shift), abi.addr(L.strength)
            for name in StokesLine.PROFILES:
                setattr(cl, name, abi.addr(getattr(L, name)))
        d = abi.lwhip_stokes()
        d.Nlines = len(st.lines)
        d.B, d.cosGamma, d.cos2chi, d.sin2chi = _ptr(st.B), _ptr(st.cosGamma), _ptr(st.cos2chi), _ptr(st.sin2chi)
        d.lines = C.cast(lines, C.POINTER(abi.lwhip_stokes_line))
        d.Quv = _ptr(self.Quv)
        d.J20 = _ptr(st.J20)
        self._stokes_keepalive = (lines, d)
        return d

    # -- normalisation / allocation of outputs -------------------------------------------------
    def _normalise_atom(self, a: AtomData):
        Ns, Nr = self.Nspace, self.Nrays
        a.n = _f64(a.n, (a.Nlevel, Ns))
        a.nStar = _f64(a.nStar, (a.Nlevel, Ns))
        a.nTotal = _f64(a.nTotal, (Ns,))
        a.vBroad = _f64(a.vBroad, (Ns,))
        if not a.detailed:
            a.Gamma = (_f64(a.Gamma, (a.Nlevel, a.Nlevel, Ns)) if a.Gamma is not None
                       else np.zeros((a.Nlevel, a.Nlevel, Ns)))
            a.C = (_f64(a.C, (a.Nlevel, a.Nlevel, Ns)) if a.C is not None
                   else np.zeros((a.Nlevel, a.Nlevel, Ns)))
        for t in a.trans:
            if not (0 <= t.Nblue < t.Nred <= self.Nlambda):
                raise ValueError('transition wavelength range outside the global grid')
            t.wavelength = _f64(t.wavelength, (t.Nlambda,))
            if not np.array_equal(t.wavelength, self.wavelength[t.Nblue:t.Nred]):
                raise ValueError('transition grid must equal wavelength[Nblue:Nred]')
            if t.Nlambda < 2:
                raise ValueError('a transition needs at least two wavelength points')
            if t.type == abi.LINE:
                t.phi = (_f64(t.phi, (t.Nlambda, Nr, 2, Ns)) if t.phi is not None
                         else np.zeros((t.Nlambda, Nr, 2, Ns)))
                t.wphi = _f64(t.wphi, (Ns,)) if t.wphi is not None else np.zeros(Ns)
                t.aDamp = _f64(t.aDamp, (Ns,)) if t.aDamp is not None else np.zeros(Ns)
                if t.rhoPrd is not None:
                    t.rhoPrd = _f64(t.rhoPrd, (t.Nlambda, Ns))
                t.Qelast = _f64(t.Qelast, (Ns,)) if t.Qelast is not None else np.zeros(Ns)
            else:
                t.alpha = _f64(t.alpha, (t.Nlambda,))
            t.Rij = np.zeros(Ns)
            t.Rji = np.zeros(Ns)

    @property
    def activeAtoms(self):
        return [a for a in self.atoms if not a.detailed]

    @property
    def detailedAtoms(self):
        return [a for a in self.atoms if a.detailed]

    def gamma_prefill(self, crsw=1.0):
        """Gamma <- crsw * C, the host pre-fill of LwContext.formal_sol_gamma_matrices
        (Source/LwMiddleLayer.pyx:3198-3203)."""
        for a in self.activeAtoms:
            a.Gamma[...] = crsw * a.C

    # -- flattening ------------------------------------------------------------------------------
    def _boundary(self, b: Boundary, keep):
        out = abi.lwhip_boundary()
        out.type = int(b.type)
        out.Nmu = 0
        if b.type == abi.BC_CALLABLE:
            idxs = np.ascontiguousarray(b.idxs, dtype=np.int32)
            data = _f64(b.bcData)
            nd = 3 if self.grid2d is not None else 2      # 2D: [Nlambda, Nmu, Nx] (FormalScalar2d.cpp:930-938)
            if idxs.shape != (self.Nrays, 2) or data.ndim != nd or data.shape[0] != self.Nlambda \
                    or (nd == 3 and data.shape[2] != self.grid2d.Nx):
                raise ValueError('CALLABLE boundary needs idxs[Nrays,2] and bcData[Nlambda,Nmu] (2D: [Nlambda,Nmu,Nx])')
            b.idxs, b.bcData = idxs, data
            keep += [idxs, data]
            out.Nmu = data.shape[1]
            out.idxs = idxs.ctypes.data_as(abi.i32p)
            out.bcData = _ptr(data)
        return out

    def descriptor(self) -> abi.lwhip_problem:
        """Build the flat C descriptor.  The returned struct borrows this object's arrays: keep
        the Problem alive for as long as any library context created from it."""
        keep = []
        atoms = (abi.lwhip_atom * len(self.atoms))()
        for ia, a in enumerate(self.atoms):
            trans = (abi.lwhip_transition * max(len(a.trans), 1))()
            keep.append(trans)
            adr = abi.addr
            for kr, t in enumerate(a.trans):
                ct = abi.raw_view(trans[kr])    # (pointer fields take integer addresses: half the time of typed pointers)
                ct.type, ct.i, ct.j = int(t.type), int(t.i), int(t.j)
                ct.Nblue, ct.Nred = int(t.Nblue), int(t.Nred)
                ct.prd = 1 if (t.type == abi.LINE and t.rhoPrd is not None) else 0
                ct.Aji, ct.Bji, ct.Bij = float(t.Aji), float(t.Bji), float(t.Bij)
                ct.lambda0, ct.dopplerWidth = float(t.lambda0), float(t.dopplerWidth)
                ct.wavelength = adr(t.wavelength)
                ct.alpha = adr(t.alpha)
                ct.phi = adr(t.phi)
                ct.wphi = adr(t.wphi)
                ct.aDamp = adr(t.aDamp)
                ct.rhoPrd = adr(t.rhoPrd)
                ct.Rij = adr(t.Rij)
                ct.Rji = adr(t.Rji)
                ct.Qelast = adr(t.Qelast)
            ca = abi.raw_view(atoms[ia])
            ca.Nlevel, ca.Ntrans, ca.detailed = int(a.Nlevel), len(a.trans), int(bool(a.detailed))
            ca.n = adr(a.n)
            ca.nStar = adr(a.nStar)
            ca.nTotal = adr(a.nTotal)
            ca.vBroad = adr(a.vBroad)
            ca.Gamma = adr(a.Gamma)
            ca.C = adr(a.C)
            ca.trans = C.addressof(trans)
        p = abi.lwhip_problem()
        p.abiVersion = abi.ABI_VERSION
        p.Nspace, p.Nrays, p.Nlambda = self.Nspace, self.Nrays, self.Nlambda
        p.Natom = len(self.atoms)
        p.formalSolver = self.formalSolver
        p.storeDepthData = int(self.storeDepthData)
        p.height = _ptr(self.height)
        p.temperature = _ptr(self.temperature)
        p.vlosMu = _ptr(self.vlosMu)
        p.muz = _ptr(self.muz)
        p.wmu = _ptr(self.wmu)
        p.wavelength = _ptr(self.wavelength)
        p.zLowerBc = self._boundary(self.zLowerBc, keep)
        p.zUpperBc = self._boundary(self.zUpperBc, keep)
        p.bgChi, p.bgEta, p.bgSca = _ptr(self.bgChi), _ptr(self.bgEta), _ptr(self.bgSca)
        p.J, p.I = _ptr(self.J), _ptr(self.I)
        p.depthChi, p.depthEta, p.depthI = (_ptr(self.depthChi), _ptr(self.depthEta),
                                            _ptr(self.depthI))
        p.atoms = C.cast(atoms, C.POINTER(abi.lwhip_atom))
        keep.append(atoms)
        if self.grid2d is not None:
            g = self.grid2d.descriptor()
            keep.append(g)
            p.grid2d = C.cast(C.pointer(g), C.c_void_p)
        self._keepalive = keep
        return p

    # -- convenience -----------------------------------------------------------------------------
    def copy(self) -> 'Problem':
        import copy
        new = copy.deepcopy(self)
        new._keepalive = None
        return new

    def outputs(self):
        """Dict of the arrays an iteration writes (copies)."""
        out = {'J': self.J.copy(), 'I': self.I.copy()}
        for ia, a in enumerate(self.atoms):
            if not a.detailed:
                out[f'Gamma{ia}'] = a.Gamma.copy()
            out[f'n{ia}'] = a.n.copy()
            for kr, t in enumerate(a.trans):
                out[f'Rij{ia}_{kr}'] = t.Rij.copy()
                out[f'Rji{ia}_{kr}'] = t.Rji.copy()
        return out

    def __deepcopy__(self, memo):
        import copy
        cls = self.__class__
        new = cls.__new__(cls)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            if k in ('_keepalive', '_stokes_keepalive'):
                setattr(new, k, None)
            else:
                setattr(new, k, copy.deepcopy(v, memo))
        return new


def check_mus(mus):
    """`mus` of compute_rays / observer_problem as a float64 vector of direction cosines in (0, 1]."""
    mus = np.ascontiguousarray(np.atleast_1d(np.asarray(mus, dtype=np.float64)).reshape(-1))
    if mus.size == 0 or not np.all((mus > 0.0) & (mus <= 1.0)):
        raise ValueError('mus must be direction cosines in (0, 1]')
    return mus


def grid_active_transitions(prob: Problem, wavelengths):
    """The active set of a new wavelength grid, SpectrumConfiguration.subset_configuration (lightweaver/atomic_set.py:209-257):
    with Nb = searchsorted(old, w[0]) and Nr = min(searchsorted(old, w[-1]) + 1, Nlambda), a transition is active iff its rows
    [Nblue, Nred) of the old grid meet [Nb, Nr).  Returns {(atomIdx, transIdx): bool} in the order of prob.atoms."""
    w = _f64(np.atleast_1d(wavelengths))
    Nb = int(np.searchsorted(prob.wavelength, w[0]))
    Nr = min(int(np.searchsorted(prob.wavelength, w[-1])) + 1, prob.Nlambda)
    return {(ia, kr): max(Nb, t.Nblue) < min(Nr, t.Nred)
            for ia, a in enumerate(prob.atoms) for kr, t in enumerate(a.trans)}


def _interp_rows(xNew, xOld, f):
    """numpy.interp along the first axis of f [len(xOld), Nspace], depth by depth: linear, the end values held outside."""
    out = np.empty((xNew.shape[0], f.shape[1]))
    for k in range(f.shape[1]):
        out[:, k] = np.interp(xNew, xOld, f[:, k])
    return out


def _observer_regrid(prob: Problem, new: Problem, Nr, wavelengths, background, contAlpha, lowerBc):
    """`new` (observer_problem's copy of `prob` with Nr rays) moved onto the grid `wavelengths`: what the reference's second
    context holds after compute_rays(wavelengths, mus) (LwMiddleLayer.pyx:1960-1963, :2770-2774, :3866)."""
    w = _f64(np.atleast_1d(wavelengths)).copy()
    if w.ndim != 1 or w.shape[0] < 2 or not np.all(np.isfinite(w)) or not np.all(np.diff(w) > 0.0):
        raise ValueError('observer_problem: wavelengths must be at least two finite, strictly increasing values')
    if background is None or len(background) != 3:
        raise ValueError('observer_problem: wavelengths needs background=(chi, eta, sca), each [Nwave, Nspace]')
    Nw, Ns = w.shape[0], prob.Nspace
    active = grid_active_transitions(prob, w)
    contAlpha = {(int(k[0]), int(k[1])): v for k, v in (contAlpha or {}).items()}
    new.wavelength = w
    new.Nlambda = Nw
    new.bgChi, new.bgEta, new.bgSca = (_f64(a, (Nw, Ns)).copy() for a in background)
    new.J = _interp_rows(w, prob.wavelength, prob.J)
    new.I = np.zeros((Nw, Nr))
    if new.storeDepthData:
        new.depthChi, new.depthEta, new.depthI = (np.zeros((Nw, Nr, 2, Ns)) for _ in range(3))
    for ia, a in enumerate(new.atoms):
        kept = []
        for kr, t in enumerate(a.trans):
            if not active[(ia, kr)]:
                continue    # (for formal_sol an inactive transition and a missing one are the same)
            old = prob.atoms[ia].trans[kr]
            t.Nblue, t.Nred = 0, Nw
            t.wavelength = w.copy()
            if t.type == abi.LINE:
                t.phi = np.zeros((Nw, Nr, 2, Ns))
                if old.rhoPrd is not None:
                    t.rhoPrd = _interp_rows(w, old.wavelength, old.rhoPrd)
            else:
                if (ia, kr) not in contAlpha:
                    raise ValueError(f'observer_problem: contAlpha has no cross-section for the active continuum {(ia, kr)}')
                t.alpha = _f64(contAlpha[(ia, kr)], (Nw,)).copy()
            kept.append(t)
        a.trans = kept
    if new.zLowerBc.type == abi.BC_CALLABLE:
        new.zLowerBc.bcData = _f64(lowerBc, (Nw, Nr)).copy()


def observer_problem(prob: Problem, mus, vz=None, wmu=None, lowerBc=None, stokes=False, mux=None, muy=None,
                     wavelengths=None, background=None, contAlpha=None) -> Problem:
    """The problem LwContext.compute_rays (Source/LwMiddleLayer.pyx:3898-4002) hands to its second context: a deep copy
    of `prob` (populations, J, background, rhoPrd: equal, not shared) whose rays are `mus`, with wmu = 0 as
    Atmosphere.rays leaves it unless `wmu` is given, and vlosMu = mu (x) v_z.  `vz` [Nspace] defaults to
    vlosMu[0] / muz[0] of `prob` (the 1D convention vlosMu = muz (x) v_z).  Every line's phi is dropped for a zero array of
    the new ray count (make it with compute_profiles); full-Stokes data is not carried over unless `stokes` (below).  A
    CALLABLE lower boundary
    has no data for a new direction: pass `lowerBc` [Nlambda, Nmu] (it feeds the up-going rays); a CALLABLE upper
    boundary becomes ZERO, which an up-going ray never reads.  What Context.compute_rays computes on the device without any
    of this is formal_sol(upOnly=True) of this problem.
    stokes: the copy carries StokesData for the new rays, as compute_rays(mus, stokes=True) of the reference leaves its
    second context: B, gammaB, chiB and every line's Zeeman components equal to the originals (not shared), zero polarised
    profiles of the new ray count (make them with compute_polarised_profiles) and the field projected onto the new
    directions (update_projections).  `mux` / `muy` [Nmu] default to the reference's 1D convention mux = sqrt(1 - mu^2),
    muy = 0 (lightweaver/atmosphere.py:1509-1510).  Context.compute_rays(stokes=True) computes single_stokes_fs(upOnly=True)
    of this problem on the device.
    wavelengths: the problem of compute_rays(wavelengths, mus), on a grid [Nwave] of the caller's choice: the new grid, the
    `background` = (chi, eta, sca) given for it, J and every PRD line's rhoPrd by numpy.interp in wavelength per depth point
    (end values held).  The transitions active by the reference's rule (grid_active_transitions) cover the whole new grid
    (Nblue, Nred = 0, Nwave; a zero phi of the new shape; continua take `contAlpha[(atomIdx, transIdx)]` [Nwave]); the others
    are removed from their atoms.  `lowerBc` is then [Nwave, Nmu].  Not with stokes."""
    if prob.grid2d is not None:
        raise ValueError('observer_problem: 1D plane-parallel problems only')
    if wavelengths is not None and stokes:
        raise ValueError('observer_problem: stokes=True is not served on a new wavelength grid')
    if wavelengths is None and (background is not None or contAlpha is not None):
        raise ValueError('observer_problem: background / contAlpha go with wavelengths')
    mus = check_mus(mus)
    Nr, Ns = mus.shape[0], prob.Nspace
    vz = (prob.vlosMu[0] / prob.muz[0]) if vz is None else _f64(vz, (Ns,))
    new = prob.copy()
    new.muz = mus.copy()
    new.Nrays = Nr
    new.wmu = np.zeros(Nr) if wmu is None else _f64(wmu, (Nr,)).copy()
    new.vlosMu = np.ascontiguousarray(mus[:, None] * vz[None, :])
    new.I = np.zeros((prob.Nlambda, Nr))
    if new.storeDepthData:
        dshape = (prob.Nlambda, Nr, 2, Ns)
        new.depthChi, new.depthEta, new.depthI = np.zeros(dshape), np.zeros(dshape), np.zeros(dshape)
    for a in new.atoms:
        for t in a.trans:
            if t.type == abi.LINE:
                t.phi = np.zeros((t.Nlambda, Nr, 2, Ns))   # (the stored one carries the old ray count)
    if new.zLowerBc.type == abi.BC_CALLABLE:
        if lowerBc is None:
            raise ValueError('observer_problem: a CALLABLE lower boundary has no data for new directions: pass lowerBc '
                             '[Nlambda, Nmu]')
        idxs = np.full((Nr, 2), -1, dtype=np.int32)
        idxs[:, 1] = np.arange(Nr)
        NlaBc = prob.Nlambda if wavelengths is None else np.size(wavelengths)
        new.zLowerBc = Boundary(abi.BC_CALLABLE, idxs=idxs, bcData=_f64(lowerBc, (NlaBc, Nr)).copy())
    if new.zUpperBc.type == abi.BC_CALLABLE:
        new.zUpperBc = Boundary(abi.BC_ZERO)
    new.stokes = None
    new.Quv = None
    if wavelengths is not None:
        _observer_regrid(prob, new, Nr, wavelengths, background, contAlpha, lowerBc)
    if stokes:
        st = prob.stokes
        if st is None:
            raise ValueError('observer_problem: stokes=True needs Problem.set_stokes(StokesData(...)) first')
        mux, muy = observer_azimuth(mus, mux, muy)
        new.set_stokes(StokesData(B=st.B.copy(), gammaB=st.gammaB.copy(), chiB=st.chiB.copy(), mux=mux, muy=muy,
                                  lines=[StokesLine(L.atom, L.trans, L.alpha.copy(), L.shift.copy(), L.strength.copy())
                                         for L in st.lines], vz=vz.copy()))
    return new


def observer_problem_2d(prob: Problem, muz, mux=None, vz=None, vx=None, lowerBc=None, grid2d_factory=None) -> Problem:
    """observer_problem for a 2D problem: what LwContext.compute_rays (Source/LwMiddleLayer.pyx:3898-4002) hands to its second
    context.  A deep copy of `prob` whose rays are the directions (muz, mux) with wmu = 0, the intersection table of those
    directions (grid2d.build_grid2d, or grid2d_factory(x, z, mux, muz, temperature) -> Grid2d), vlosMu = mux (x) vx +
    muz (x) vz, a zero phi [Nlambda, Nmu, 2, Nspace] per line (make it with compute_profiles) and I [Nlambda, Nmu, Nx].
    `mux` defaults to sqrt(1 - muz^2); `vz` [Nspace] is required, `vx` defaults to zeros.  A CALLABLE upper boundary becomes
    ZERO (an up-going ray never reads it), a CALLABLE lower one takes `lowerBc` [Nlambda, Nmu, Nx].  What
    Context.compute_rays_2d computes on the device without any of this is formal_sol(upOnly=True) of this problem."""
    from .grid2d import build_grid2d
    g = prob.grid2d
    if g is None:
        raise ValueError('observer_problem_2d: 2D problems only (observer_problem serves 1D ones)')
    if not g.periodic:
        raise ValueError('observer_problem_2d: fixed x boundaries have no data for new directions')
    muz = check_mus(muz)
    Nr, Ns = muz.shape[0], prob.Nspace
    mux = np.sqrt(1.0 - muz ** 2) if mux is None else _f64(np.atleast_1d(mux), muz.shape).copy()
    if np.any(muz ** 2 + mux ** 2 > 1.0 + 1e-12):
        raise ValueError('observer_problem_2d: muz^2 + mux^2 > 1')
    if vz is None:
        raise ValueError('observer_problem_2d: vz [Nspace] is required')
    vz = _f64(np.asarray(vz).reshape(-1), (Ns,))
    vx = np.zeros(Ns) if vx is None else _f64(np.asarray(vx).reshape(-1), (Ns,))
    new = prob.copy()
    new.muz = muz.copy()
    new.Nrays = Nr
    new.wmu = np.zeros(Nr)
    new.vlosMu = np.ascontiguousarray(mux[:, None] * vx[None, :] + muz[:, None] * vz[None, :])
    new.I = np.zeros((prob.Nlambda, Nr, g.Nx))
    if new.storeDepthData:
        dshape = (prob.Nlambda, Nr, 2, Ns)
        new.depthChi, new.depthEta, new.depthI = np.zeros(dshape), np.zeros(dshape), np.zeros(dshape)
    for a in new.atoms:
        for t in a.trans:
            if t.type == abi.LINE:
                t.phi = np.zeros((t.Nlambda, Nr, 2, Ns))   # (the stored one carries the old ray count)
    zLow, zUp = g.zLowerBc, g.zUpperBc
    if new.zLowerBc.type == abi.BC_CALLABLE:
        if lowerBc is None:
            raise ValueError('observer_problem_2d: a CALLABLE lower boundary has no data for new directions: pass lowerBc '
                             '[Nlambda, Nmu, Nx]')
        idxs = np.full((Nr, 2), -1, dtype=np.int32)
        idxs[:, 1] = np.arange(Nr)
        new.zLowerBc = Boundary(abi.BC_CALLABLE, idxs=idxs, bcData=_f64(lowerBc, (prob.Nlambda, Nr, g.Nx)).copy())
    if new.zUpperBc.type == abi.BC_CALLABLE:
        new.zUpperBc = Boundary(abi.BC_ZERO)
        zUp = abi.BC_ZERO
    make = grid2d_factory if grid2d_factory is not None else build_grid2d
    ng = make(g.x.copy(), g.z.copy(), mux.copy(), muz.copy(), g.temperature.copy())
    ng.zLowerBc, ng.zUpperBc = zLow, zUp
    new.grid2d = ng
    new.stokes = None
    new.Quv = None
    return new


def observer_azimuth(mus, mux=None, muy=None):
    """mux, muy [Nmu] of observer directions `mus`: the reference's 1D convention mux = sqrt(1 - mu^2), muy = 0
    (lightweaver/atmosphere.py:1509-1510) where not given."""
    mus = check_mus(mus)
    mux = np.sqrt(1.0 - mus ** 2) if mux is None else _f64(np.atleast_1d(mux), mus.shape).copy()
    muy = np.zeros(mus.shape[0]) if muy is None else _f64(np.atleast_1d(muy), mus.shape).copy()
    return mux, muy
