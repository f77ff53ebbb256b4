"""1.5D column batches (BASELINE.json configs[3]): many independent plane-parallel columns, each a
Context-equivalent problem with its own atmosphere, profiles and populations.  Columns never
exchange radiation, so they shard across GPUs with NO collective ("replicas"): rank r simply owns
columns r, r + world, ....  On one GPU the columns' contexts are all resident in HBM (26 MB of phi
per H + Ca II column at ~3k wavelengths: thousands fit in 288 GB) and their iterations are queued
back to back on one stream, so the device never idles between columns; profiles are regenerated on
the device per column (lwhip_compute_profiles), so phi never crosses PCIe.
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence

from . import _abi as abi
from .context import Context, _check
from .model import Problem


@dataclass
class BatchConvergence:
    """What ColumnBatch.iterate_to_convergence returns, one entry per column."""
    iterations: List[int]     # the value iterate_ctx_se would return for the column (NmaxIter - 1 where it did not converge)
    converged: List[bool]
    final: List[list]         # [JUpdate, popsUpdate] of the column's stop iteration, with prd=True also its prdUpdate ([] where it
                              # did not converge)


def _hprd_key(tables):
    """What identifies a hybrid-PRD table set given as Context's `hprd`: the address of its lwhip_hprd, whether it comes as an object
    with `.ptr` or as a ctypes pointer (two pointer objects to one lwhip_hprd are one set)."""
    import ctypes
    ptr = getattr(tables, 'ptr', tables)
    try:
        return ctypes.cast(ptr, ctypes.c_void_p).value
    except (TypeError, ctypes.ArgumentError):
        return id(tables)


def columns_of_rank(ncolumns: int, world: int, rank: int) -> List[int]:
    """Round-robin column ownership; no data-path communication between ranks."""
    if not (0 <= rank < world):
        raise ValueError('bad rank')
    return list(range(rank, ncolumns, world))


def pack_time_dep(problems, active, prevTimePops):
    """What lwhip_batch_time_dep_update takes as nOld: per ACTIVE column one contiguous array holding the [Nlevel, Nspace]
    blocks of its solved atoms back to back in atom order (prevTimePops[i]: one array per solved atom of column i), and
    NULL for the others.  Returns (the [n] pointer array, the arrays it points to, None for inactive columns)."""
    import ctypes as C
    import numpy as np
    n = len(problems)
    keep = [None] * n
    ptrs = (abi.f64p * n)()
    for i in active:
        solved = [a for a in problems[i].atoms if not a.detailed]
        prev = prevTimePops[i]
        if prev is None or len(prev) != len(solved):
            raise ValueError('time_dep_update: column %d needs one array per solved atom' % i)
        blocks = []
        for a, p in zip(solved, prev):
            p = np.asarray(p, dtype=np.float64)
            if p.shape != (a.Nlevel, problems[i].Nspace):
                raise ValueError('time_dep_update: column %d: prevTimePops of %s must be [Nlevel, Nspace]' % (i, a.name))
            blocks.append(p.reshape(-1))
        keep[i] = np.ascontiguousarray(np.concatenate(blocks)) if blocks else np.zeros(1)
        ptrs[i] = keep[i].ctypes.data_as(abi.f64p)
    return ptrs, keep


def pack_nr_args(n, active, atoms, stages, backgroundNe, ne, dC=None, nPrev=None, dt=0.0, crsw=1.0):
    """What lwhip_batch_nr_post_update takes as perColumn: [n] lwhip_nr_args, those of the ACTIVE columns filled by
    _abi.make_nr_args (shared `atoms` and `stages`; backgroundNe, ne, dC, nPrev one entry per column; crsw a scalar or one
    value per column), the others zeroed.  Returns (the array, what it points to)."""
    arr = (abi.lwhip_nr_args * n)()
    keep = [None] * n
    per = lambda a, i: None if a is None else a[i]  # noqa: E731
    for i in active:
        cr = crsw[i] if isinstance(crsw, (list, tuple)) else crsw
        args, k = abi.make_nr_args(atoms, stages, backgroundNe[i], ne[i], dC=per(dC, i), nPrev=per(nPrev, i), dt=dt, crsw=cr)
        arr[i] = args
        keep[i] = (args, k)
    return arr, keep


class ColumnBatch:
    _ng = None         # (Norder, Nperiod, Ndelay) in effect, Ndelay after the max rule -- configure_ng; None: no Ng acceleration

    def __init__(self, problems: Sequence[Problem], device: int = 0, stream: Optional[int] = None,
                 device_profiles: bool = True, streams: Optional[Sequence[int]] = None, fused: bool = True, hprd=None):
        """hprd: hybrid PRD for every column.  True: each column builds the tables for its own velocity field on the device
        (Context(p, hprd=True)) and owns them -- close() frees them after the contexts.  A list: one table set per column (as
        Context's `hprd`), borrowed; a set given twice raises ValueError (columns on one set would share one JRest).  Either way
        they are `hprd_tables`, one entry per column, and download() brings each column's JRest into its own.  The columns'
        tile lists follow their velocities, so the fused launches take the largest workgroup count (sweep_shape).  A hybrid
        batch that the library refuses to fuse is reported with a RuntimeWarning: see `fused`.
        `fused` (default): the columns advance in ONE set of launches per iteration (lwhip_batch_*: one grid
        slice per column), which is what fills the device when a single column's wavelength grid does not;
        it needs structurally identical columns on one stream and falls back to per-column launches otherwise.
        `streams`: optional HIP streams (handles) the columns are dealt to round-robin in the per-column mode, so
        that the small reduce / apply / solve kernels of one column overlap the sweep of the next."""
        self.problems = list(problems)
        self._batch = None
        self._active = None     # (None: every column; else the increasing list of active columns -- set_active)
        if hprd is None or hprd is False:
            hp = lambda i: None     # noqa: E731
        elif hprd is True:
            hp = lambda i: True     # noqa: E731
        else:
            given = list(hprd)
            if len(given) != len(self.problems):
                raise ValueError('ColumnBatch: hprd needs one table set per column')
            keys = [_hprd_key(t) for t in given]
            if len(set(keys)) != len(keys):
                raise ValueError('ColumnBatch: a hybrid-PRD table set is given to more than one column; each column needs tables of '
                                 'its own (they hold its JRest)')
            hp = lambda i: given[i]     # noqa: E731
        if streams:
            self.contexts = [Context(p, device=device, stream=streams[i % len(streams)], hprd=hp(i))
                             for i, p in enumerate(self.problems)]
        else:
            # (the columns of a fused batch share their structure: all but the first borrow the first one's tables)
            # Columns 2 .. n are created concurrently: a borrower's lwhip_create is ~3 ms of host work (its own bookkeeping of
            # the shared structure) + ~2 ms of allocations and uploads, ctypes releases the interpreter lock for the call, and
            # the library's create path shares nothing writable between contexts (the donor's borrower count is atomic, the
            # error text is per thread).  LWHIP_CREATE_THREADS=1 creates them one after the other (default 16).
            hint = len(self.problems) if fused else 0
            # (hprd=True: every column builds its own tables inside its create, also concurrently -- lwhip_hprd_build keeps its
            # buffers in locals, takes its stream from the library's locked pool and leaves the error text per thread)
            self.contexts = ([Context(self.problems[0], device=device, stream=stream, batchHint=hint, hprd=hp(0))]
                             if self.problems else [])
            donor = self.contexts[0] if (fused and self.contexts) else None
            rest = self.problems[1:]
            # (round 6, tools/create_threads_time.py: 64 borrowers take 5.8 / 1.8 / 1.35 / 0.99 ms each on 1 / 4 / 8 / 16 threads --
            # beyond that the HIP runtime's own locks around allocations and copies are what is left)
            nthr = max(1, min(int(os.environ.get('LWHIP_CREATE_THREADS', '16')), os.cpu_count() or 1, len(rest)))
            if os.environ.get('LWHIP_DEBUG') and any(os.environ.get(k) for k in ('LWHIP_PAD_SENTINEL', 'LWHIP_TRACE_ALLOC')):
                nthr = 1    # (those diagnoses number the allocations in creation order: one creating thread)
            make = lambda ip: Context(ip[1], device=device, stream=stream, batchHint=hint, like=donor, hprd=hp(ip[0]))  # noqa: E731
            rest = list(enumerate(rest, 1))
            if nthr > 1:
                from concurrent.futures import ThreadPoolExecutor
                with ThreadPoolExecutor(max_workers=nthr) as ex:
                    futs = [ex.submit(make, p) for p in rest]
                    made, err = [], None
                    for f in futs:
                        try:
                            made.append(f.result())
                        except Exception as e:  # (close what was made, then report the first failure)
                            err = err or e
                    if err is not None:
                        for c in reversed(made):
                            c.close()
                        self.contexts[0].close()
                        raise err
                    self.contexts += made
            else:
                self.contexts += [make(p) for p in rest]
        if fused and not streams and self.contexts:
            import ctypes as C
            lib = self.contexts[0].lib
            arr = (C.c_void_p * len(self.contexts))(*[c._h for c in self.contexts])
            h = C.c_void_p()
            if lib.lwhip_batch_create(arr, len(self.contexts), C.byref(h)) == abi.OK:
                self._batch = h
            elif hprd is not None and hprd is not False:
                import warnings
                warnings.warn('ColumnBatch: the hybrid-PRD columns are not fused (%s): they advance by per-column launches'
                              % lib.lwhip_last_error().decode(errors='replace'), RuntimeWarning, stacklevel=2)
        if device_profiles:
            self.compute_profiles()

    def __len__(self):
        return len(self.contexts)

    @property
    def fused(self) -> bool:
        """Whether the columns advance in one set of launches (lwhip_batch_create accepted them)."""
        return self._batch is not None

    @property
    def hprd_tables(self):
        """Each column's hybrid-PRD tables (Context.hprd_tables; None for plain PRD), in column order."""
        return [c.hprd_tables for c in self.contexts]

    def sweep_shape(self):
        """{'columns': [(workgroups of the full sweep, of the PRD rates pass)] per column, 'launch': the two gridDim.x values
        the fused batch launches with for the current active set} (lwhip_batch_sweep_shape).  Hybrid-PRD columns differ in their
        counts and the launch takes the largest; every other batch has equal counts."""
        if self._batch is None:
            raise RuntimeError('sweep_shape: the batch is not fused')
        import numpy as np
        lib = self.contexts[0].lib
        per = np.zeros((len(self.contexts), 2), dtype=np.int32)
        launch = np.zeros(2, dtype=np.int32)
        _check(lib, lib.lwhip_batch_sweep_shape(self._batch, per.ctypes.data_as(abi.i32p), launch.ctypes.data_as(abi.i32p)),
               'lwhip_batch_sweep_shape')
        return {'columns': [(int(a), int(b)) for a, b in per], 'launch': (int(launch[0]), int(launch[1]))}

    def compute_profiles(self):
        """phi / wphi of every line of every column on the device (lwhip_batch_compute_profiles: one launch pair for
        the whole batch; per column where the batch is not fused).  After an atmosphere upload the next iteration
        does this by itself for the columns concerned."""
        if self._batch is not None:
            lib = self.contexts[0].lib
            _check(lib, lib.lwhip_batch_compute_profiles(self._batch), 'lwhip_batch_compute_profiles')
            return
        for c in self.contexts:
            c.compute_profiles(deviceResident=True)

    def sweep_instance(self):
        """Context.sweep_instance() of the fused batch's one sweep launch: plain only if every column's own launch would
        be (lwhip_batch_sweep_instance).  Not fused: the columns launch by themselves -- ask them."""
        if self._batch is None:
            raise RuntimeError('sweep_instance: the batch is not fused; see the columns\' Context.sweep_instance()')
        import ctypes as C
        lib = self.contexts[0].lib
        out = (C.c_int32 * 4)()
        _check(lib, lib.lwhip_batch_sweep_instance(self._batch, out), 'lwhip_batch_sweep_instance')
        return {'main': bool(out[0]), 'prdRates': bool(out[1]), 'lanes': bool(out[2]), 'switch': bool(out[3])}

    def close(self):
        if self._batch is not None:
            self.contexts[0].lib.lwhip_batch_destroy(self._batch)
            self._batch = None
        # (borrowers of the first column's tables before the first column; a column made with hprd=True frees its own hybrid-PRD
        # tables behind its context, the first column's once its last borrower is gone)
        for c in reversed(self.contexts):
            c.close()
        self.contexts = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def formal_sol_gamma_matrices(self, lambdaIterate=False, sync_host=True):
        """One iteration of every column; kernels of all columns are queued before the first
        result is read back.  sync_host=False reads nothing back (no host wait per column): use it for
        all but the iterations whose dJMax is wanted.  With an active set (set_active) only its columns advance and the
        entries of the others are None."""
        if self._active is not None and not self._active:
            return [None] * len(self.contexts) if sync_host else None
        if self._batch is not None:
            import ctypes as C
            from .context import IterationUpdate
            lib = self.contexts[0].lib
            crsw = self.contexts[0].crsw
            if not sync_host:
                _check(lib, lib.lwhip_batch_formal_sol_gamma_matrices(self._batch, int(lambdaIterate), crsw, None),
                       'lwhip_batch_formal_sol_gamma_matrices')
                return None
            res = (abi.lwhip_iter_result * len(self.contexts))()
            _check(lib, lib.lwhip_batch_formal_sol_gamma_matrices(self._batch, int(lambdaIterate), crsw, res),
                   'lwhip_batch_formal_sol_gamma_matrices')
            ups = [IterationUpdate(updatedJ=True, dJMax=r.dJMax, dJMaxIdx=r.dJMaxIdx, crsw=crsw) for r in res]
            return ups if self._active is None else self._only_active(ups)
        cols = [self.contexts[i] for i in self.active]
        for c in cols:
            c.gamma_prefill_from_C(c.crsw)
            c.fs_partial(lambdaIterate)
        if not sync_host:
            for c in cols:
                _check(c.lib, c.lib.lwhip_fs_finalise(c._h, None), 'lwhip_fs_finalise')
            return None
        ups = [None] * len(self.contexts)
        for i in self.active:
            ups[i] = self.contexts[i].fs_finalise()
        return ups

    def _only_active(self, per_column):
        """per_column with None in the places of the inactive columns."""
        act = set(self.active)
        return [u if i in act else None for i, u in enumerate(per_column)]

    def stat_equil(self, report=False):
        """Queued for every (active) column without a host wait in between; one status check at the end.
        report=True: returns one IterationUpdate(updatedPops=True, dPops=[...], dPopsMaxIdx=[...]) per column -- what
        Context.stat_equil gives for the column alone --, None for an inactive column (lwhip_batch_stat_equil_report: the
        columns' change records are combined on the device and come back in one copy; not fused: each column's own
        Context.stat_equil(deviceResident=True))."""
        if report:
            return self._stat_equil_report()[1]
        if self._active is not None and not self._active:
            return
        if self._batch is not None:
            lib = self.contexts[0].lib
            _check(lib, lib.lwhip_batch_stat_equil(self._batch), 'lwhip_batch_stat_equil')
            return
        if self._ng is not None:    # (a column's Ng step follows its solve and reads its result back: the reporting route)
            self._stat_equil_report()
            return
        cols = [self.contexts[i] for i in self.active]
        for c in cols:
            c.stat_equil(deviceResident=True, sync_host=False)
        for c in cols:
            c.check_status()

    def _stat_equil_report(self):
        """stat_equil(report=True): (JUpdates, popsUpdates), one entry per column, None for inactive columns.  JUpdates: on a
        fused batch the dJMax the last formal_sol_gamma_matrices left on the device, which the columns' convergence records
        carry (so that call needs no host wait of its own); None when not fused."""
        from .context import IterationUpdate
        n = len(self.contexts)
        pops = [None] * n
        if self._active is not None and not self._active:
            return None, pops
        if self._batch is None:
            for i in self.active:
                pops[i] = self.contexts[i].stat_equil(deviceResident=True)
            return None, pops
        import ctypes as C
        import numpy as np
        lib = self.contexts[0].lib
        nAct = sum(1 for a in self.problems[0].atoms if not a.detailed)
        if nAct == 0:
            for i in self.active:
                pops[i] = IterationUpdate(updatedPops=True, dPops=[], dPopsMaxIdx=[])
            return None, pops
        dPops = np.zeros((n, nAct))
        dIdx = np.zeros((n, nAct), dtype=np.int32)
        _check(lib, lib.lwhip_batch_stat_equil_report(self._batch, dPops.ctypes.data_as(abi.f64p), dIdx.ctypes.data_as(abi.i32p)),
               'lwhip_batch_stat_equil_report')
        rec = np.zeros((n, 2 + 2 * nAct))
        stride = C.c_int(0)
        _check(lib, lib.lwhip_batch_conv_records(self._batch, rec.ctypes.data_as(abi.f64p), C.byref(stride)), 'lwhip_batch_conv_records')
        assert stride.value == rec.shape[1]
        crsw = self.contexts[0].crsw
        Js = [None] * n
        # (plain lists first: this runs between two iterations with the device idle -- 512 columns, 3 ms element by element, 1 ms so)
        dP, dI, rc = dPops.tolist(), dIdx.tolist(), rec.tolist()
        # (with Ng the solve was followed by every active column's Ng step: whether it extrapolated is the device's word)
        acc = self.ng_state()['lastAccelerated'] if self._ng is not None else [False] * n
        for i in self.active:
            pops[i] = IterationUpdate(updatedPops=True, dPops=dP[i], dPopsMaxIdx=dI[i], ngAccelerated=acc[i])
            Js[i] = IterationUpdate(updatedJ=True, dJMax=rc[i][0], dJMaxIdx=int(rc[i][1]), crsw=crsw)
        return Js, pops

    # -- Ng acceleration: every column as a lone Context with configure_ng ---------------------------------------------------
    def configure_ng(self, Norder=0, Nperiod=0, Ndelay=0):
        """Context.configure_ng for every column (NgOptions; struct Ng, Source/Ng.hpp): each column keeps its own history and
        its own call count, seeded with its current populations -- all columns, active or not.  From then on stat_equil
        runs each active column's Ng step after its solve and reports Ng's max_change, taken after any extrapolation.
        Fused: lwhip_batch_ng_configure -- histories and counts on the device, one launch for the active columns.  Not
        fused: each column's own Context.configure_ng.  (0, 0, 0) turns it off again; a repeated call seeds again."""
        No, Np, Nd = int(Norder), int(Nperiod), int(Ndelay)
        off = (No, Np, Nd) == (0, 0, 0)
        if self._batch is not None:
            lib = self.contexts[0].lib
            _check(lib, lib.lwhip_batch_ng_configure(self._batch, No, Np, Nd), 'lwhip_batch_ng_configure')
        else:
            for c in self.contexts:
                c.configure_ng(No, Np, Nd)
                if off:
                    c._ng = None    # (the column's stat_equil takes its plain route again)
        self._ng = None if off else (No, Np, max(Nd, Np + 2))

    def ng_state(self):
        """{'options': (Norder, Nperiod, Ndelay) in effect (Ndelay after the max rule) or None when off, 'counts': every
        column's Ng call count (1 after configure_ng), 'lastAccelerated': whether its last Ng step extrapolated}: the device's
        own words -- fused: lwhip_batch_ng_state; not fused: each column's Context.ng_state."""
        n = len(self.contexts)
        if self._batch is None:
            if self._ng is None:
                return dict(options=None, counts=[0] * n, lastAccelerated=[False] * n)
            sts = [c.ng_state() for c in self.contexts]
            return dict(options=self._ng, counts=[s['count'] for s in sts], lastAccelerated=[s['lastAccelerated'] for s in sts])
        import ctypes as C
        import numpy as np
        lib = self.contexts[0].lib
        opts = (C.c_int32 * 3)()
        counts = np.zeros(n, dtype=np.int32)
        last = np.zeros(n, dtype=np.int32)
        _check(lib, lib.lwhip_batch_ng_state(self._batch, opts, counts.ctypes.data_as(abi.i32p), last.ctypes.data_as(abi.i32p)),
               'lwhip_batch_ng_state')
        o = tuple(opts)
        return dict(options=None if o == (0, 0, 0) else o, counts=counts.tolist(), lastAccelerated=[bool(x) for x in last])

    def ng_accelerate(self):
        """The Ng step alone on the active columns, from the populations now on the device (fused:
        lwhip_batch_ng_accelerate, one launch; not fused: each column's lwhip_ng_accelerate): one
        IterationUpdate(updatedPops=True, dPops, dPopsMaxIdx, ngAccelerated) per active column, None for the others."""
        import numpy as np
        from .context import IterationUpdate
        if self._ng is None:
            raise RuntimeError('ng_accelerate before configure_ng')
        n = len(self.contexts)
        ups = [None] * n
        if self._active is not None and not self._active:
            return ups
        nAct = sum(1 for a in self.problems[0].atoms if not a.detailed)
        acc = np.zeros(n, dtype=np.int32)
        dPops = np.zeros((n, max(nAct, 1)))
        dIdx = np.zeros((n, max(nAct, 1)), dtype=np.int32)
        if self._batch is not None:
            lib = self.contexts[0].lib
            _check(lib, lib.lwhip_batch_ng_accelerate(self._batch, acc.ctypes.data_as(abi.i32p), dPops.ctypes.data_as(abi.f64p),
                                                      dIdx.ctypes.data_as(abi.i32p)), 'lwhip_batch_ng_accelerate')
        else:
            for i in self.active:
                c = self.contexts[i]
                a1 = np.zeros(max(nAct, 1), dtype=np.int32)
                _check(c.lib, c.lib.lwhip_ng_accelerate(c._h, a1.ctypes.data_as(abi.i32p), dPops[i].ctypes.data_as(abi.f64p),
                                                        dIdx[i].ctypes.data_as(abi.i32p)), 'lwhip_ng_accelerate')
                acc[i] = int(a1[:nAct].any())
        for i in self.active:
            ups[i] = IterationUpdate(updatedPops=True, dPops=dPops[i, :nAct].tolist(), dPopsMaxIdx=dIdx[i, :nAct].tolist(),
                                     ngAccelerated=bool(acc[i]))
        return ups

    # -- time-dependent and charge-conserving updates: every active column in one launch -------------------------------------
    def _solved(self):
        return [ia for ia, a in enumerate(self.problems[0].atoms) if not a.detailed]

    def _pops_reports(self, atoms, run):
        """One IterationUpdate per column (None for inactive ones) from run(dPops [n, Nsolved], dIdx [n, Nsolved]), which
        fills the rows of the active columns; `atoms`: the atoms the call updated, whose entries are reported."""
        import numpy as np
        from .context import IterationUpdate
        n, solved = len(self.contexts), self._solved()
        dPops = np.zeros((n, max(len(solved), 1)))
        dIdx = np.zeros((n, max(len(solved), 1)), dtype=np.int32)
        run(dPops, dIdx)
        pos = [solved.index(ia) for ia in atoms]
        ups = [None] * n
        for i in self.active:
            ups[i] = IterationUpdate(updatedPops=True, dPops=[float(dPops[i, q]) for q in pos],
                                     dPopsMaxIdx=[int(dIdx[i, q]) for q in pos])
        return ups

    def _unfused_pops(self, atoms, update):
        """The per-column route of time_dep_update / nr_post_update: update(i, context) on every active column's own Context,
        reported by _rel_diff_pops of downloads taken before and after."""
        import numpy as np
        ups = [None] * len(self.contexts)
        for i in self.active:
            c = self.contexts[i]
            c.download(abi.POPS)
            before = [np.array(c.prob.atoms[ia].n, dtype=np.float64, copy=True) for ia in atoms]
            update(i, c)
            c.download(abi.POPS)
            ups[i] = c._rel_diff_pops(atoms, before)
        return ups

    def time_dep_update(self, dt, prevTimePops):
        """Context.time_dep_update(dt, prevTimePops[i], deviceResident=True) of every active column: dt a scalar or one value
        per column, prevTimePops[i] the list of [Nlevel, Nspace] arrays of column i's solved atoms (entries of inactive
        columns may be None).  Fused: lwhip_batch_time_dep_update -- one launch for all columns and atoms, the columns' changes
        combined on the device.  Returns one IterationUpdate(updatedPops=True, dPops, dPopsMaxIdx) per column (rel_diff_pops of
        the reference: the change against the populations before the call), None for an inactive column."""
        import numpy as np
        n = len(self.contexts)
        if self._active is not None and not self._active:
            return [None] * n
        dts = np.ascontiguousarray(np.broadcast_to(np.asarray(dt, dtype=np.float64), (n,)))
        solved = self._solved()
        if self._batch is None:
            return self._unfused_pops(solved, lambda i, c: c.time_dep_update(float(dts[i]), prevTimePops[i], deviceResident=True))
        if not solved:
            return self._pops_reports([], lambda dP, dI: None)
        ptrs, keep = pack_time_dep(self.problems, self.active, prevTimePops)
        lib = self.contexts[0].lib
        return self._pops_reports(solved, lambda dP, dI: _check(
            lib, lib.lwhip_batch_time_dep_update(self._batch, ptrs, dts.ctypes.data_as(abi.f64p), dP.ctypes.data_as(abi.f64p),
                                                 dI.ctypes.data_as(abi.i32p)), 'lwhip_batch_time_dep_update'))

    def nr_post_update(self, stages, backgroundNe, ne, dC=None, nPrev=None, dt=0.0, atoms=None):
        """Context.nr_post_update(..., deviceResident=True) of every active column: `stages` and `atoms` are shared,
        backgroundNe, ne, dC and nPrev are lists with one entry per column (those of inactive columns may be None); ne[i] is
        updated in place.  Fused: lwhip_batch_nr_post_update.  Returns one IterationUpdate(updatedPops=True, dPops,
        dPopsMaxIdx) per column with one entry per listed atom, None for an inactive column."""
        n = len(self.contexts)
        if self._active is not None and not self._active:
            return [None] * n
        if atoms is None:
            atoms = self._solved()
        atoms = [int(ia) for ia in atoms]
        per = lambda a, i: None if a is None else a[i]  # noqa: E731
        if self._batch is None:
            return self._unfused_pops(atoms, lambda i, c: c.nr_post_update(stages, backgroundNe[i], ne[i], dC=per(dC, i),
                                                                           nPrev=per(nPrev, i), dt=dt, atoms=atoms,
                                                                           deviceResident=True))
        arr, keep = pack_nr_args(n, self.active, atoms, stages, backgroundNe, ne, dC=dC, nPrev=nPrev, dt=dt,
                                 crsw=[c.crsw for c in self.contexts])
        lib = self.contexts[0].lib
        return self._pops_reports(atoms, lambda dP, dI: _check(
            lib, lib.lwhip_batch_nr_post_update(self._batch, arr, dP.ctypes.data_as(abi.f64p), dI.ctypes.data_as(abi.i32p)),
            'lwhip_batch_nr_post_update'))

    # -- PRD sub-iterations: every active column as a lone Context's prd_redistribute ----------------------------------------
    def prd_redistribute(self, maxIter=3, tol=1e-2):
        """Context.prd_redistribute(maxIter, tol, deviceResident=True) of every active column: each column runs its own
        sub-iterations and stops after the first whose own largest |d rho / rho| is below tol, whatever the others do.  Fused:
        lwhip_batch_redistribute_prd -- one set of launches per sub-iteration for all columns, the stopping rule per column
        on the device, one copy back per group of four sub-iterations (a batch on the ray-column march: the columns one after
        the other inside that call).  Not fused: each column's own call.  Returns one IterationUpdate per column with
        NprdSubIter, dRho [NprdSubIter, Nprd], dRhoMaxIdx, dJPrdMax, dJPrdMaxIdx, dJMax, dJMaxIdx; None for an inactive
        column."""
        import numpy as np
        from .context import IterationUpdate
        n = len(self.contexts)
        ups = [None] * n
        if self._active is not None and not self._active:
            return ups
        if self._batch is None:
            for i in self.active:
                ups[i] = self.contexts[i].prd_redistribute(maxIter=maxIter, tol=tol, deviceResident=True)
            return ups
        lib = self.contexts[0].lib
        m = max(int(maxIter), 1)
        Nprd = max(self.contexts[0].Nprd, 1)
        nSub = np.zeros(n, dtype=np.int32)
        dRho = np.zeros((n, m, Nprd))
        dRhoIdx = np.zeros((n, m, Nprd), dtype=np.int32)
        dJ = np.zeros((n, m))
        dJIdx = np.zeros((n, m), dtype=np.int32)
        res = abi.lwhip_batch_prd_result(0, 0, nSub.ctypes.data_as(abi.i32p), dRho.ctypes.data_as(abi.f64p),
                                         dRhoIdx.ctypes.data_as(abi.i32p), dJ.ctypes.data_as(abi.f64p), dJIdx.ctypes.data_as(abi.i32p))
        _check(lib, lib.lwhip_batch_redistribute_prd(self._batch, int(maxIter), float(tol), res), 'lwhip_batch_redistribute_prd')
        k = res.Nprd
        for i in self.active:
            it = int(nSub[i])
            ups[i] = IterationUpdate(updatedRho=it > 0, updatedJ=it > 0, NprdSubIter=it,
                                     dRho=dRho[i, :it, :k].copy(), dRhoMaxIdx=dRhoIdx[i, :it, :k].copy(),
                                     dJPrdMax=dJ[i, :it].copy(), dJPrdMaxIdx=dJIdx[i, :it].copy(),
                                     dJMax=float(dJ[i, it - 1]) if it else 0.0, dJMaxIdx=int(dJIdx[i, it - 1]) if it else 0)
        return ups

    # -- the active set: the columns formal_sol_gamma_matrices and stat_equil advance ---------------------------------------
    @property
    def active(self) -> List[int]:
        """The columns formal_sol_gamma_matrices / stat_equil advance, increasing."""
        return list(range(len(self.contexts))) if self._active is None else list(self._active)

    def set_active(self, columns=None):
        """Only `columns` (a strictly increasing list of column indices; None: all) are advanced by formal_sol_gamma_matrices
        and stat_equil from now on (lwhip_batch_set_active; kept here where the batch is not fused).  An inactive
        ("retired") column's device state stays exactly what its last iteration left; every other method -- profiles,
        Stokes, compute_rays, download -- keeps acting on all columns; and what a column computes does not depend on which
        others are active.  An empty list: those two calls do nothing."""
        n = len(self.contexts)
        cols = None if columns is None else [int(i) for i in columns]
        if cols is not None and (any(not (0 <= i < n) for i in cols) or any(b <= a for a, b in zip(cols, cols[1:]))):
            raise ValueError('set_active: a strictly increasing list of column indices below %d' % n)
        if cols is not None and len(cols) == n:
            cols = None
        if self._batch is not None and (cols is None or cols):
            import numpy as np
            lib = self.contexts[0].lib
            arr = np.asarray(cols if cols is not None else [], dtype=np.int32)
            _check(lib, lib.lwhip_batch_set_active(self._batch, arr.ctypes.data_as(abi.i32p) if cols is not None else None,
                                                   len(arr)), 'lwhip_batch_set_active')
        self._active = cols

    def iterate_to_convergence(self, Nscatter: int = 3, NmaxIter: int = 2000, JTol: float = 5e-3, popsTol: float = 1e-3,
                               retire: bool = True, callback: Optional[Callable] = None, ng: Optional[tuple] = None,
                               prd: bool = False, prdIterTol: float = 1e-2, maxPrdSubIter: int = 3, rhoTol: Optional[float] = None):
        """iterate_ctx_se (iterate.py; lightweaver/iterate_ctx.py:85-208) for every column at once, each column judged by its
        own numbers: a column is converged at the first iteration it >= Nscatter whose own dJMax < JTol and max dPops <
        popsTol (DefaultConvergenceCriteria).  retire=True: it leaves the active set at once, so its state stays what that
        iteration left and the launches shrink; retire=False: it is only recorded and keeps iterating.  Starts from all
        columns; ends when every column has converged or after NmaxIter iterations, and restores the full active set
        before returning (also when an exception passes through).
        Returns BatchConvergence(iterations, converged, final): per column what iterate_ctx_se would return for it alone
        (NmaxIter - 1 where it did not converge), whether it converged, and its final [JUpdate, popsUpdate] ([] where it
        did not).  callback(it, JUpdates, popsUpdates, active): per-column lists (None for columns inactive in that
        iteration; popsUpdates None while it < Nscatter) and the active set after the iteration's retirements.
        ng: (Norder, Nperiod, Ndelay) -- configure_ng with them once all columns are active, before the first iteration;
        None leaves the batch as it is configured.  With Ng each column's popsUpdate carries its own ngAccelerated, and a
        retired column's history and call count stay frozen with the rest of its state.
        prd: each iteration it >= Nscatter is formal solution, reported solve, then prd_redistribute(maxPrdSubIter, prdIterTol),
        and each column is judged by DefaultConvergenceCriteria(..., rhoTol).is_converged(J, pops, prdUpdate) as iterate_ctx_se
        judges it; the `final` of a converged column then carries the PRD update as third element, and the callback gets the
        per-column PRD updates (None while it < Nscatter) as a fifth argument.
        No time-dependent or charge-conserving updates here."""
        from .iterate import DefaultConvergenceCriteria
        n = len(self.contexts)
        convs = [DefaultConvergenceCriteria(c, JTol, popsTol, rhoTol if prd else None) for c in self.contexts]
        extra = lambda prdUps: (prdUps,) if prd else ()    # (the callback's trailing argument, only with prd)  # noqa: E731
        out = BatchConvergence(iterations=[max(NmaxIter - 1, 0)] * n, converged=[False] * n, final=[[] for _ in range(n)])
        pending = list(range(n))
        self.set_active(None)
        if ng is not None:
            self.configure_ng(*ng)
        try:
            for it in range(NmaxIter):
                if not pending:
                    break
                # (fused: the reported solve brings this iteration's dJMax back with the population changes -- one host wait)
                solve = it >= Nscatter
                want = callback is not None if not solve else self._batch is None
                JUps = self.formal_sol_gamma_matrices(sync_host=want)
                if not solve:
                    if callback is not None:
                        callback(it, JUps, None, self.active, *extra(None))
                    continue
                recJ, pUps = self._stat_equil_report()
                if JUps is None:
                    JUps = recJ
                rUps = self.prd_redistribute(maxIter=maxPrdSubIter, tol=prdIterTol) if prd else [None] * n
                new = [i for i in pending if convs[i].is_converged(JUps[i], pUps[i], rUps[i])]
                for i in new:
                    out.iterations[i], out.converged[i] = it, True
                    out.final[i] = [JUps[i], pUps[i]] + ([rUps[i]] if prd else [])
                if new:
                    pending = [i for i in pending if not out.converged[i]]
                    if retire:
                        self.set_active(pending)
                if callback is not None:
                    callback(it, JUps, pUps, self.active, *extra(rUps))
        finally:
            self.set_active(None)
        return out

    def iterate(self, niter: int, nscatter: int = 3, callback: Optional[Callable] = None):
        """iterate_ctx_se-style loop (lightweaver/iterate_ctx.py:157-176) over the whole batch."""
        ups = []
        for it in range(niter):
            want = callback is not None or it == niter - 1
            ups = self.formal_sol_gamma_matrices(sync_host=want)
            if it >= nscatter:
                self.stat_equil()
            if callback is not None:
                callback(it, ups)
        return ups

    # -- full Stokes (every column with its own prob.stokes, the polarised lines of the first column) -----------------------
    def compute_polarised_profiles(self, deviceResident=True):
        """Context.compute_polarised_profiles of every column: phi, wphi and phiQ..psiV of the polarised lines, all columns'
        lines in one launch list (lwhip_batch_compute_polarised_profiles; per column where the batch is not fused).  Each
        column's prob.stokes is attached first, with its J20 when it holds one; downloaded unless deviceResident."""
        if self._batch is None:
            for c in self.contexts:
                c.compute_polarised_profiles(deviceResident=deviceResident)
            return
        fresh = [c._stokes_attach(c.prob.stokes.J20 if c.prob.stokes is not None else None) for c in self.contexts]
        if not deviceResident:
            for c, f in zip(self.contexts, fresh):
                c.upload(abi.ATMOS | abi.NSTAR | (0 if f else abi.STOKES))
        lib = self.contexts[0].lib
        _check(lib, lib.lwhip_batch_compute_polarised_profiles(self._batch), 'lwhip_batch_compute_polarised_profiles')
        if not deviceResident:
            for c in self.contexts:
                c.download(abi.PROFILES | abi.STOKES)

    def single_stokes_fs(self, updateJ=False, upOnly=True, deviceResident=False, sync_host=True):
        """Context.single_stokes_fs of every column in one set of launches (lwhip_batch_full_stokes_fs): fills each column's
        prob.I and prob.Quv, with updateJ also its J (and J20).  A column's J20 is its prob.stokes.J20 (None: an ordinary
        call).  Returns one IterationUpdate per column, or None when sync_host is False.  Not deviceResident: each column's
        inputs go up and its outputs come back as Context.single_stokes_fs moves them.  An unfused batch runs the columns
        one after the other."""
        if self._batch is None:
            ups = [c.single_stokes_fs(updateJ=updateJ, upOnly=upOnly, J20=c.prob.stokes.J20 if c.prob.stokes is not None else None,
                                      deviceResident=deviceResident) for c in self.contexts]
            return ups if sync_host else None
        import ctypes as C
        from .context import IterationUpdate
        fresh = [c._stokes_attach(c.prob.stokes.J20 if c.prob.stokes is not None else None) for c in self.contexts]
        if not deviceResident:
            for c, f in zip(self.contexts, fresh):
                c.upload(abi.J | abi.POPS | abi.BC | abi.RHOPRD | (0 if f else abi.STOKES))
        lib = self.contexts[0].lib
        res = (abi.lwhip_iter_result * len(self.contexts))() if sync_host else None
        _check(lib, lib.lwhip_batch_full_stokes_fs(self._batch, int(bool(updateJ)), int(bool(upOnly)), res),
               'lwhip_batch_full_stokes_fs')
        if not deviceResident:
            for c in self.contexts:
                c.download(abi.I | abi.STOKES | (abi.J if updateJ else 0))
        if not sync_host:
            return None
        return [IterationUpdate(updatedJ=bool(updateJ), dJMax=r.dJMax if updateJ else 0.0,
                                dJMaxIdx=r.dJMaxIdx if updateJ else 0, crsw=c.crsw) for r, c in zip(res, self.contexts)]

    # -- emergent spectra along observer rays ------------------------------------------------------------------------------
    def compute_rays(self, mus=1.0, laStart=0, laEnd=0, vz=None, lowerBc=None, depthData=False, stokes=False, mux=None,
                     muy=None, wavelengths=None, background=None, contAlpha=None):
        """Context.compute_rays of every column from its device-resident state, all columns in one set of launches and
        one copy back (lwhip_batch_compute_rays; an unfused batch runs the columns one after the other).  The same
        directions and wavelength range for every column; `vz` / `lowerBc`: None, or one array per column.  Returns I
        [Ncolumns, Nla, Nmu], or with depthData a RaysResult whose I, chi, eta, Idepth carry the column axis first.
        stokes: Context.compute_rays(stokes=True) of every column (lwhip_batch_compute_stokes_rays): [Ncolumns, 4, Nla, Nmu].
        wavelengths: Context.compute_rays(wavelengths=...) of every column (lwhip_batch_compute_rays_grid): one grid [Nwave]
        for all columns; `background` a list of (chi, eta, sca) and `contAlpha` a list of dicts, one per column."""
        import ctypes as C
        import numpy as np
        from .context import RaysResult
        n = len(self.contexts)
        per = lambda a, i: None if a is None else a[i]  # noqa: E731
        if stokes:
            if wavelengths is not None:
                raise ValueError('compute_rays: stokes=True is not served on a new wavelength grid')
            if background is not None or contAlpha is not None:
                raise ValueError('compute_rays: background / contAlpha go with wavelengths')
            if depthData:
                raise ValueError('compute_rays: no depthData with stokes=True')
            reqs = [c._stokes_rays_request(mus, laStart, laEnd, per(vz, i), per(lowerBc, i), mux, muy)
                    for i, c in enumerate(self.contexts)]
            if self._batch is not None:
                lib = self.contexts[0].lib
                arr = (abi.lwhip_stokes_rays * n)(*[q for q, _, _ in reqs])
                _check(lib, lib.lwhip_batch_compute_stokes_rays(self._batch, arr), 'lwhip_batch_compute_stokes_rays')
            else:
                for c, (q, _, _) in zip(self.contexts, reqs):
                    _check(c.lib, c.lib.lwhip_compute_stokes_rays(c._h, C.byref(q)), 'lwhip_compute_stokes_rays')
            return np.stack([o for _, o, _ in reqs]) if reqs else np.zeros((0, 4, 0, 0))
        return self._rays_call('', mus, laStart, laEnd, vz, lowerBc, depthData, wavelengths, background, contAlpha)

    def compute_rays_hprd(self, mus=1.0, laStart=0, laEnd=0, vz=None, lowerBc=None, depthData=False, wavelengths=None,
                          background=None, contAlpha=None):
        """Context.compute_rays_hprd of every column of a batch made with hprd=True, which compute_rays refuses
        (lwhip_batch_compute_rays_hprd / lwhip_batch_compute_rays_grid_hprd; an unfused batch runs the columns one after
        the other).  Arguments, per-column lists and results are compute_rays's; each column's rho is interpolated for its
        own velocity field.  A column retired with set_active is served from the state of its stop iteration."""
        return self._rays_call('_hprd', mus, laStart, laEnd, vz, lowerBc, depthData, wavelengths, background, contAlpha)

    def _rays_call(self, sfx, mus, laStart, laEnd, vz, lowerBc, depthData, wavelengths, background, contAlpha):
        """compute_rays (sfx '') / compute_rays_hprd (sfx '_hprd') of every column, on the stored grid or a new one."""
        import ctypes as C
        n = len(self.contexts)
        per = lambda a, i: None if a is None else a[i]  # noqa: E731
        if wavelengths is not None:
            if laStart or laEnd:
                raise ValueError('compute_rays: laStart / laEnd select rows of the context\'s own grid: leave them 0 with wavelengths')
            if background is None or len(background) != n or (contAlpha is not None and len(contAlpha) != n):
                raise ValueError('compute_rays: wavelengths needs background and contAlpha per column')
            kind, one, many = abi.lwhip_rays_grid, 'lwhip_compute_rays_grid' + sfx, 'lwhip_batch_compute_rays_grid' + sfx
            reqs = [c._rays_grid_request(mus, wavelengths, background[i], per(contAlpha, i), per(vz, i), per(lowerBc, i),
                                         depthData) for i, c in enumerate(self.contexts)]
        else:
            if background is not None or contAlpha is not None:
                raise ValueError('compute_rays: background / contAlpha go with wavelengths')
            kind, one, many = abi.lwhip_rays, 'lwhip_compute_rays' + sfx, 'lwhip_batch_compute_rays' + sfx
            reqs = [c._rays_request(mus, laStart, laEnd, per(vz, i), per(lowerBc, i), depthData)
                    for i, c in enumerate(self.contexts)]
        if self._batch is not None:
            lib = self.contexts[0].lib
            arr = (kind * n)(*[q for q, _, _ in reqs])
            _check(lib, getattr(lib, many)(self._batch, arr), many)
        else:
            for c, (q, _, _) in zip(self.contexts, reqs):
                _check(c.lib, getattr(c.lib, one)(c._h, C.byref(q)), one)
        return self._stack_rays([o for _, o, _ in reqs], depthData)

    @staticmethod
    def _stack_rays(outs, depthData):
        """The columns' RaysResults with the column axis first."""
        import numpy as np
        from .context import RaysResult
        I = np.stack([o.I for o in outs]) if outs else np.zeros((0, 0, 0))
        if not depthData:
            return I
        return RaysResult(I=I, mus=outs[0].mus, laStart=outs[0].laStart, laEnd=outs[0].laEnd,
                          chi=np.stack([o.chi for o in outs]), eta=np.stack([o.eta for o in outs]),
                          Idepth=np.stack([o.Idepth for o in outs]))

    def download(self, mask=abi.ALL_OUTPUTS | abi.POPS):
        for c in self.contexts:
            c.download(mask)
