"""Hybrid PRD tables built on the device: `build_hprd(prob)` <- LwContext.configure_hprd_coeffs
(Source/LwMiddleLayer.pyx:3686-3690 -> configure_hprd_coeffs, Source/Prd.cpp:697-946) over lwhip_hprd_build.

`Context(prob, hprd=True)` calls it; on its own it serves a caller who wants the tables (to look at them, or to hand one set
to several contexts through `Context(prob, hprd=tables)`).  There is no CPU path: without a gfx950 device it raises."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _abi as abi

_J_DT = np.dtype([('frac', np.float64), ('idx', np.int32), ('_pad', np.int32)])
_RHO_DT = np.dtype([('i0', np.int32), ('i1', np.int32), ('frac', np.float64)])


def _records(ptr, n, dt):
    """n records of dtype dt at a ctypes pointer, as a numpy view (no copy)."""
    if n == 0:
        return np.zeros(0, dtype=dt)
    raw = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), (n * dt.itemsize,))
    return np.frombuffer(raw, dtype=dt)


class HprdTables:
    """numpy views of a library-owned lwhip_hprd and the descriptor itself (`.ptr`: what lwhip_options.hprd takes).  The views
    are valid until close(); close the contexts that borrow the tables first."""

    def __init__(self, lib, ptr, prob):
        self._lib, self.ptr = lib, ptr
        h = ptr.contents
        Ns, Nrays = prob.Nspace, prob.Nrays
        as_np = np.ctypeslib.as_array
        self.NprdLambda, self.NhPrd, self.Nlines = int(h.NprdLambda), int(h.NhPrd), int(h.Nlines)
        self.prdIdxs = as_np(h.prdIdxs, (self.NprdLambda,))
        self.hPrdIdxs = as_np(h.hPrdIdxs, (max(self.NhPrd, 1),))[:self.NhPrd]
        self.JRest = as_np(h.JRest, (self.NprdLambda, Ns))
        ncell = self.NhPrd * Nrays * 2 * Ns
        self.jCoeffOff = as_np(h.jCoeffOff, (ncell + 1,))
        jc = _records(h.jCoeffs, int(self.jCoeffOff[-1]), _J_DT)
        self.jFrac, self.jIdx = jc['frac'], jc['idx']
        self.lineAtom = as_np(h.lineAtom, (self.Nlines,))
        self.lineTrans = as_np(h.lineTrans, (self.Nlines,))
        self.rho = []
        for q in range(self.Nlines):
            t = prob.atoms[int(self.lineAtom[q])].trans[int(self.lineTrans[q])]
            rc = _records(h.rhoCoeffs[q], (t.Nred - t.Nblue) * Nrays * 2 * Ns, _RHO_DT)
            self.rho.append((rc['i0'], rc['i1'], rc['frac']))

    @property
    def nbytes(self):
        """Bytes of the tables the build brought back from the device (jCoeffOff, jCoeffs, the rho tables)."""
        return int(self.jCoeffOff.nbytes + self.jFrac.size * _J_DT.itemsize
                   + sum(r[0].size for r in self.rho) * _RHO_DT.itemsize)

    def close(self):
        if self.ptr:
            self._lib.lwhip_hprd_free(self.ptr)
            self.ptr = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def build_hprd(prob, device: int = 0, includeDetailed: bool = False, stream: Optional[int] = None,
               lib_path: Optional[str] = None) -> Optional[HprdTables]:
    """The hybrid PRD tables of `prob` for its current vlosMu, built on `device` (on `stream`, or a stream of the library's).
    includeDetailed: the PRD lines of detailed atoms follow those of the active ones (what `prdDetailed` contexts need).
    None when the problem has no PRD line (the reference then stays plain PRD).  A new velocity field means new tables and a
    new context."""
    from .context import load_library
    lib = load_library(lib_path)
    # (a live Context of `prob` reads the arrays its own descriptor keeps alive: this call's descriptor must not replace them)
    prev = getattr(prob, '_keepalive', None)
    desc = prob.descriptor()
    mine, prob._keepalive = prob._keepalive, prev   # (`mine` lives until the call below has returned)
    return build_from_descriptor(lib, desc, prob, device, includeDetailed, stream)


def build_from_descriptor(lib, desc, prob, device=0, includeDetailed=False, stream=None) -> Optional[HprdTables]:
    """build_hprd for a descriptor of `prob` the caller already holds (Context: the one it creates the context from)."""
    from .context import _check
    opts = abi.lwhip_options()
    opts.device = device
    opts.stream = stream
    out = C.POINTER(abi.lwhip_hprd)()
    _check(lib, lib.lwhip_hprd_build(C.byref(desc), C.byref(opts), int(bool(includeDetailed)), C.byref(out)), 'lwhip_hprd_build')
    return HprdTables(lib, out, prob) if out else None
