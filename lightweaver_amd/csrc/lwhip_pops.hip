// lwhip_pops.hip -- population updates: statistical equilibrium, the time-dependent (backward Euler)
// update and the Newton-Raphson charge-conservation step.  One thread per depth point; every
// variant assembles a small dense system and solves it with the reference's solver:
// Crout LU with implicit row scaling and partial pivoting + one residual-correction pass
// (solve_lin_eq / lu_decompose / lu_backsub, Source/LuSolve.cpp:8-132).  The systems are tiny
// (N = Nlevel for statistical equilibrium and the time-dependent update, 1 <= N <= 32; N = sum Nlevel + 1
// <= 64 for the Newton-Raphson step), so this is latency-, not throughput-bound (< 1 % of an
// iteration); coalescing comes from the depth index being the fastest axis of every array.
// Two paths:
//  - registers, 2 <= N <= 6 (SOLVE_REG_MAXN): d_solve_lin_eq_reg<N> of lwhip_lu.h, one unrolled instantiation
//    per N picked by a switch; stat_eq and time_dep only (the NR system is assembled in LDS at every size);
//  - LDS, N = 1 and N >= 7, and every NR system: d_solve_lin_eq below on a per-thread workspace of
//    2 N^2 + 5 N doubles.  The block size is the largest power of two <= 64 whose workspaces fit 150 KB
//    (solve_block_threads: 64 threads up to N = 11, 32 up to 16, 16 up to 23, 8 up to 33, 4 up to 47, 2 up to
//    64); above 48 KB the kernel's dynamic-LDS limit is raised first (solve_set_lds).  A stat_eq launch takes
//    block size and LDS from its largest atom; smaller atoms take the register path inside those blocks.
// Both paths, every register instantiation and every block-size class (11, 13, 21, 32, 40 and 64 equations) are
// tested against the oracle and an extended-precision solution (tests/test_pops_levels.py).
#include "lwhip_device.h"
#include "../../include/lwhip.h"

// These systems are ill conditioned at large dt / strong rates (kappa up to ~1e8), so rounding-level
// differences are amplified to 1e-9 .. 1e-7 in the populations.  No fused multiply-adds here: the
// operations then match the reference's (and the oracle's) one for one, and so do the results.
#pragma clang fp contract(off)

#include "lwhip_lu.h"

namespace lwhip
{
// Per-thread workspace in LDS: element e of thread t lives at base[e * stride + t] (stride = block
// size), so the threads of a wavefront never collide on a bank and the dynamically indexed rows of
// the pivoting LU cost an LDS access instead of a scratch (HBM-backed) one.
struct LdsVec
{
    double* p;
    int stride;
    DEVINL double& operator[](int e) const { return p[(size_t)e * stride]; }
};
// doubles of workspace per thread for an N x N system: A, A0 (N^2 each), b, b0, res, vv, index (N each)
__host__ __device__ inline size_t solve_ws_doubles(int N) { return (size_t)2 * N * N + 5 * N; }
struct SolveWs
{
    LdsVec A, A0, b, b0, res, vv, index;
    DEVINL SolveWs(double* base, int N, int stride, int tid)
    {
        double* q = base + tid;
        A = { q, stride };
        q += (size_t)N * N * stride;
        A0 = { q, stride };
        q += (size_t)N * N * stride;
        b = { q, stride };
        q += (size_t)N * stride;
        b0 = { q, stride };
        q += (size_t)N * stride;
        res = { q, stride };
        q += (size_t)N * stride;
        vv = { q, stride };
        q += (size_t)N * stride;
        index = { q, stride };
    }
};

// solve A x = b in place (x returned in b); A is destroyed.  Returns false for a singular matrix
// (an all-zero row, where the reference throws "Singular Matrix", LuSolve.cpp:22-23).
DEVINL bool d_solve_lin_eq(int N, const SolveWs& w)
{
    const LdsVec& A = w.A;
    for (int i = 0; i < N; ++i)
    {
        w.b0[i] = w.b[i];
        for (int j = 0; j < N; ++j)
            w.A0[i * N + j] = A[i * N + j];
    }
    // lu_decompose :8-70
    bool singular = false;
    for (int i = 0; i < N; ++i)
    {
        double big = 0.0;
        for (int j = 0; j < N; ++j)
            big = fmax(big, fabs(A[i * N + j]));
        if (big == 0.0)
            singular = true;
        w.vv[i] = 1.0 / big;
    }
    if (singular)
        return false;
    for (int j = 0; j < N; ++j)
    {
        for (int i = 0; i < j; ++i)
        {
            double sum = A[i * N + j];
            for (int q = 0; q < i; ++q)
                sum -= A[i * N + q] * A[q * N + j];
            A[i * N + j] = sum;
        }
        int iMax = 0;
        double big = 0.0;
        for (int i = j; i < N; ++i)
        {
            double sum = A[i * N + j];
            for (int q = 0; q < j; ++q)
                sum -= A[i * N + q] * A[q * N + j];
            A[i * N + j] = sum;
            const double cand = w.vv[i] * fabs(sum);
            if (big < cand)
            {
                iMax = i;
                big = cand;
            }
        }
        if (j != iMax)
        {
            for (int q = 0; q < N; ++q)
            {
                const double tmp = A[iMax * N + q];
                A[iMax * N + q] = A[j * N + q];
                A[j * N + q] = tmp;
            }
            w.vv[iMax] = w.vv[j];
        }
        w.index[j] = (double)iMax;
        if (A[j * N + j] == 0.0)
            A[j * N + j] = 1e-20;
        const double tmp = 1.0 / A[j * N + j];
        for (int i = j + 1; i < N; ++i)
            A[i * N + j] *= tmp;
    }
    // lu_backsub :72-101
    auto backsub = [&](const LdsVec& x) {
        int ii = -1;
        for (int i = 0; i < N; ++i)
        {
            const int ip = (int)w.index[i];
            double sum = x[ip];
            x[ip] = x[i];
            if (ii >= 0)
            {
                for (int j = ii; j < i; ++j)
                    sum -= A[i * N + j] * x[j];
            }
            else if (sum != 0.0)
            {
                ii = i;
            }
            x[i] = sum;
        }
        for (int i = N - 1; i >= 0; --i)
        {
            double sum = x[i];
            for (int j = i + 1; j < N; ++j)
                sum -= A[i * N + j] * x[j];
            x[i] = sum / A[i * N + i];
        }
    };
    backsub(w.b);
    // one pass of iterative improvement :114-131
    for (int i = 0; i < N; ++i)
    {
        double r = w.b0[i];
        for (int j = 0; j < N; ++j)
            r -= w.A0[i * N + j] * w.b[j];
        w.res[i] = r;
    }
    backsub(w.res);
    for (int i = 0; i < N; ++i)
        w.b[i] += w.res[i];
    return true;
}


enum { SOLVE_REG_MAXN = 6 };

// threads per block such that the workspace fits the LDS (a power of two between 1 and 64)
static int solve_block_threads(int N)
{
    const size_t budget = 150 * 1024;
    int tb = 64;
    while (tb > 1 && solve_ws_doubles(N) * sizeof(double) * tb > budget)
        tb >>= 1;
    return tb;
}
static hipError_t solve_set_lds(const void* fn, size_t lds)
{
    if (lds > 48 * 1024)
        return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    return hipSuccess;
}

// max |(new - old) / new| over the populations a block has just updated, with the flattened [level, depth]
// index of its first occurrence (Ng::max_change, Source/Ng.hpp:138-156, which LwContext.stat_equil /
// time_dep_update report as dPops): one (value, index) pair per block, combined on the host.
DEVINL void report_change(double best, int bestIdx, double* out /* [gridDim.x][2] of this atom, or null */)
{
    if (!out)
        return;
    __shared__ double sV[64];
    __shared__ int sI[64];
    sV[threadIdx.x] = best;
    sI[threadIdx.x] = bestIdx;
    __syncthreads();
    if (threadIdx.x == 0)
    {
        double v = 0.0;
        int idx = 0x7fffffff;
        for (int q = 0; q < (int)blockDim.x; ++q)
            if (sV[q] > v || (sV[q] == v && sV[q] > 0.0 && sI[q] < idx))
            {
                v = sV[q];
                idx = sI[q];
            }
        out[2 * blockIdx.x] = v;
        out[2 * blockIdx.x + 1] = (v > 0.0) ? (double)idx : 0.0;
    }
}

// ---- stat_eq_impl: Source/UpdatePopulations.cpp:7-47 -------------------------------------------------------
// one depth point of an atom with N <= 6 levels, the system in registers
template <int N>
DEVINL bool stat_eq_point_reg(double* n, const double* Gamma, const double nTot, const int Ns, const int k, double& best, int& bestIdx)
{
    double A[N][N], b[N], old[N];
    // Gamma_k and the elimination row: the level with the largest population
    int iElim = 0;
    double nMax = 0.0;
#pragma unroll
    for (int i = 0; i < N; ++i)
    {
        old[i] = n[(size_t)i * Ns + k];
        if (nMax < old[i])
        {
            iElim = i;
            nMax = old[i];
        }
    }
#pragma unroll
    for (int i = 0; i < N; ++i)
    {
#pragma unroll
        for (int j = 0; j < N; ++j)
        {
            const double g = Gamma[((size_t)i * N + j) * Ns + k];
            A[i][j] = (i == iElim) ? 1.0 : g;
        }
        b[i] = (i == iElim) ? nTot : 0.0;
    }
    if (!d_solve_lin_eq_reg<N>(A, b))
        return false;
#pragma unroll
    for (int i = 0; i < N; ++i)
    {
        const double cur = b[i];
        n[(size_t)i * Ns + k] = cur;
        if (cur != 0.0)
        {
            const double change = fabs((cur - old[i]) / cur);
            if (change > best)
            {
                best = change;
                bestIdx = i * Ns + k;
            }
        }
    }
    return true;
}

// blockIdx.y selects the atom, so every active atom is solved by one launch
template <class A> DEVINL void stat_eq_body(const A& a)
{
    extern __shared__ double lds[];
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    const int Ns = a.Ns;
    const NrAtom at = a.atoms[blockIdx.y];
    const int N = at.Nlevel;
    double best = 0.0;
    int bestIdx = 0x7fffffff;
    if (k >= a.k0 && k < a.k1 && N >= 2 && N <= SOLVE_REG_MAXN)
    {
        double* n = a.n + (size_t)at.levelOff * Ns;
        const double* Gamma = a.Gamma + at.gammaOff;
        const double nTot = a.nTotal[(size_t)at.atom * Ns + k];
        bool ok = true;
        switch (N)
        {
        case 2: ok = stat_eq_point_reg<2>(n, Gamma, nTot, Ns, k, best, bestIdx); break;
        case 3: ok = stat_eq_point_reg<3>(n, Gamma, nTot, Ns, k, best, bestIdx); break;
        case 4: ok = stat_eq_point_reg<4>(n, Gamma, nTot, Ns, k, best, bestIdx); break;
        case 5: ok = stat_eq_point_reg<5>(n, Gamma, nTot, Ns, k, best, bestIdx); break;
        default: ok = stat_eq_point_reg<6>(n, Gamma, nTot, Ns, k, best, bestIdx); break;
        }
        if (!ok)
            atomicExch(a.status, LWHIP_ERR_SINGULAR);
    }
    else if (k >= a.k0 && k < a.k1)
    {
        double* n = a.n + (size_t)at.levelOff * Ns;
        const double* Gamma = a.Gamma + at.gammaOff;
        const SolveWs w(lds, N, blockDim.x, threadIdx.x);
        // Gamma_k and the elimination row: the level with the largest population
        int iElim = 0;
        double nMax = 0.0;
        for (int i = 0; i < N; ++i)
        {
            const double ni = n[(size_t)i * Ns + k];
            if (nMax < ni)
            {
                iElim = i;
                nMax = ni;
            }
            for (int j = 0; j < N; ++j)
                w.A[i * N + j] = Gamma[((size_t)i * N + j) * Ns + k];
        }
        for (int i = 0; i < N; ++i)
        {
            w.A[iElim * N + i] = 1.0;
            w.b[i] = 0.0;
        }
        w.b[iElim] = a.nTotal[(size_t)at.atom * Ns + k];
        if (!d_solve_lin_eq(N, w))
            atomicExch(a.status, LWHIP_ERR_SINGULAR);
        else
        {
            for (int i = 0; i < N; ++i)
            {
                const double cur = w.b[i];
                const double old = n[(size_t)i * Ns + k];
                n[(size_t)i * Ns + k] = cur;
                if (cur != 0.0)
                {
                    const double change = fabs((cur - old) / cur);
                    if (change > best)
                    {
                        best = change;
                        bestIdx = i * Ns + k;
                    }
                }
            }
        }
    }
    report_change(best, bestIdx, a.change ? a.change + (size_t)blockIdx.y * 2 * gridDim.x : nullptr);
}

// BATCH: column batches -- blockIdx.z picks the column's argument block (read through the constant address space)
// (blocks of at most 64 threads -- solve_block_threads --: the register form of the 6 x 6 solve may use the whole file)
template <bool BATCH> __global__ void __launch_bounds__(64) stat_eq_kernel(const StatEqArgs a0, const StatEqArgs* __restrict__ list)
{
    dbg_poison_lds();
    if constexpr (BATCH)
        stat_eq_body(CTAB(StatEqArgs, list)[blockIdx.z]);
    else
        stat_eq_body(a0);
}

int stat_eq_blocks(int Ns, int maxNlevel)
{
    const int tb = solve_block_threads(maxNlevel);
    return (Ns + tb - 1) / tb;
}

hipError_t launch_stat_eq(const StatEqArgs& a, int maxNlevel, hipStream_t stream, const StatEqArgs* list, int nBatch)
{
    if (maxNlevel > 64 || a.Natoms <= 0)
        return hipErrorInvalidValue;
    const int tb = solve_block_threads(maxNlevel);
    const size_t lds = solve_ws_doubles(maxNlevel) * sizeof(double) * tb;
    hipError_t e = solve_set_lds(list ? (const void*)stat_eq_kernel<true> : (const void*)stat_eq_kernel<false>, lds);
    if (e != hipSuccess)
        return e;
    if (list)
        LWHIP_LAUNCH(stat_eq_kernel<true>, dim3((a.Ns + tb - 1) / tb, a.Natoms, nBatch > 0 ? nBatch : 1), dim3(tb), lds, stream, a,
                           list);
    else
        LWHIP_LAUNCH(stat_eq_kernel<false>, dim3((a.Ns + tb - 1) / tb, a.Natoms), dim3(tb), lds, stream, a, list);
    return hipGetLastError();
}

// ---- column batches: one convergence record per column -----------------------------------------------------
// One wavefront per active column.  Per solved atom it combines the column's nBlocks (value, index) pairs of report_change
// by the rule of Ng::max_change (Source/Ng.hpp:138-156; the host loop of stat_equil_impl for one context): the largest
// value, the first flattened [level, depth] index among equal values, index 0 for the value 0.  Lane l takes blocks l,
// l + 64, ...; the lanes' candidates meet in a butterfly (the rule does not depend on the order of combination).  The record
// [dJMax, idx, dPops_0, idx_0, ...] goes to the row of the column's ORIGINAL number, so one copy of `rec` reports all columns.
__global__ void __launch_bounds__(64) batch_conv_kernel(const BatchConvArgs a)
{
    dbg_poison_lds();
    const int col = a.cols ? a.cols[blockIdx.x] : (int)blockIdx.x;
    double* rec = a.rec + (size_t)col * (2 + 2 * a.Natoms);
    for (int q = 0; q < a.Natoms; ++q)
    {
        const double* ch = a.change + ((size_t)col * a.Natoms + q) * a.nBlocks * 2;
        double v = 0.0;
        int idx = 0x7fffffff;
        for (int b = threadIdx.x; b < a.nBlocks; b += 64)
        {
            const double x = ch[2 * b];
            const int i = (int)ch[2 * b + 1];
            if (x > v || (x == v && x > 0.0 && i < idx))
            {
                v = x;
                idx = i;
            }
        }
        for (int s = 32; s > 0; s >>= 1)
        {
            const double ov = __shfl_xor(v, s);
            const int oi = __shfl_xor(idx, s);
            if (ov > v || (ov == v && oi < idx))
            {
                v = ov;
                idx = oi;
            }
        }
        if (threadIdx.x == 0)
        {
            rec[2 + 2 * q] = v;
            rec[3 + 2 * q] = (v > 0.0) ? (double)idx : 0.0;
        }
    }
    if (threadIdx.x == 0)
    {
        rec[0] = a.tail[2 * (size_t)col];
        rec[1] = a.tail[2 * (size_t)col + 1];
    }
}

hipError_t launch_batch_conv(const BatchConvArgs& a, int nActive, hipStream_t stream)
{
    if (nActive < 1 || a.Natoms < 1 || a.nBlocks < 1)
        return hipErrorInvalidValue;
    LWHIP_LAUNCH(batch_conv_kernel, dim3(nActive), dim3(64), 0, stream, a);
    return hipGetLastError();
}

// ---- time_dependent_update_impl: Source/UpdatePopulations.cpp:120-151 --------------------------------------
// The per-point code below is shared by the lone kernels and the column-batch ones.  The batched kernels report the change of
// what they update (report_change: a barrier), so nothing in these bodies returns early: a thread outside the depth range, or
// whose system is singular, skips its work by predicate and contributes best = 0, bestIdx = 0x7fffffff; every thread of a block
// reaches every barrier.  `old` is read just before n is overwritten: no second copy of the populations.
template <int N>
DEVINL bool time_dep_point_reg(double* n, const double* nOld, const double* Gamma, const double dt, const int Ns, const int k,
                               double& best, int& bestIdx)
{
    double A[N][N], b[N];
#pragma unroll
    for (int i = 0; i < N; ++i)
    {
        b[i] = nOld[(size_t)i * Ns + k];
#pragma unroll
        for (int j = 0; j < N; ++j)
        {
            const double g = Gamma[((size_t)i * N + j) * Ns + k];
            A[i][j] = (i == j) ? 1.0 - g * dt : -g * dt;
        }
    }
    if (!d_solve_lin_eq_reg<N>(A, b))
        return false;
#pragma unroll
    for (int i = 0; i < N; ++i)
    {
        const double cur = b[i];
        const double old = n[(size_t)i * Ns + k];
        n[(size_t)i * Ns + k] = cur;
        if (cur != 0.0)
        {
            const double change = fabs((cur - old) / cur);
            if (change > best)
            {
                best = change;
                bestIdx = i * Ns + k;
            }
        }
    }
    return true;
}

// one atom of N levels: n, nOld, Gamma are the atom's own; change: its [gridDim.x][2] pairs, or null (then no barrier is met)
DEVINL void time_dep_body(const int N, const int Ns, const int k0, const int k1, double* n, const double* nOld, const double* Gamma,
                          const double dt, int* status, double* change)
{
    extern __shared__ double lds[];
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    const bool inRange = k >= k0 && k < k1;
    double best = 0.0;
    int bestIdx = 0x7fffffff;
    if (inRange && N >= 2 && N <= SOLVE_REG_MAXN)
    {
        bool ok = true;
        switch (N)
        {
        case 2: ok = time_dep_point_reg<2>(n, nOld, Gamma, dt, Ns, k, best, bestIdx); break;
        case 3: ok = time_dep_point_reg<3>(n, nOld, Gamma, dt, Ns, k, best, bestIdx); break;
        case 4: ok = time_dep_point_reg<4>(n, nOld, Gamma, dt, Ns, k, best, bestIdx); break;
        case 5: ok = time_dep_point_reg<5>(n, nOld, Gamma, dt, Ns, k, best, bestIdx); break;
        default: ok = time_dep_point_reg<6>(n, nOld, Gamma, dt, Ns, k, best, bestIdx); break;
        }
        if (!ok)
            atomicExch(status, LWHIP_ERR_SINGULAR);
    }
    else if (inRange)
    {
        const SolveWs w(lds, N, blockDim.x, threadIdx.x);
        for (int i = 0; i < N; ++i)
        {
            w.b[i] = nOld[(size_t)i * Ns + k];
            for (int j = 0; j < N; ++j)
                w.A[i * N + j] = -Gamma[((size_t)i * N + j) * Ns + k] * dt;
            w.A[i * N + i] = 1.0 - Gamma[((size_t)i * N + i) * Ns + k] * dt;
        }
        if (!d_solve_lin_eq(N, w))
            atomicExch(status, LWHIP_ERR_SINGULAR);
        else
        {
            for (int i = 0; i < N; ++i)
            {
                const double cur = w.b[i];
                const double old = n[(size_t)i * Ns + k];
                n[(size_t)i * Ns + k] = cur;
                if (cur != 0.0)
                {
                    const double change1 = fabs((cur - old) / cur);
                    if (change1 > best)
                    {
                        best = change1;
                        bestIdx = i * Ns + k;
                    }
                }
            }
        }
    }
    report_change(best, bestIdx, change);
}

// BATCH: column batches -- blockIdx.z picks the column's argument block (read through the constant address space), blockIdx.y
// the solved atom, so all solved atoms of all active columns go in one launch; every depth point is solved.  The atom's rows
// of nOld follow those of the atoms before it.  The lone form is launched once per atom.
template <bool BATCH>
__global__ void __launch_bounds__(64) time_dep_kernel(int N, int Ns, int k0, int k1, double* n, const double* nOld, const double* Gamma,
                                                      double dt, int* status, const TimeDepArgs* __restrict__ list)
{
    dbg_poison_lds();
    if constexpr (BATCH)
    {
        const TimeDepArgs a = ld_c(CTAB(TimeDepArgs, list) + blockIdx.z);
        int rows = 0;
        for (int q = 0; q < (int)blockIdx.y; ++q)
            rows += a.atoms[q].Nlevel;
        const NrAtom at = a.atoms[blockIdx.y];
        time_dep_body(at.Nlevel, a.Ns, 0, a.Ns, a.n + (size_t)at.levelOff * a.Ns, a.nOld + (size_t)rows * a.Ns, a.Gamma + at.gammaOff, a.dt,
                      a.status, a.change ? a.change + (size_t)blockIdx.y * 2 * gridDim.x : nullptr);
    }
    else
        time_dep_body(N, Ns, k0, k1, n, nOld, Gamma, dt, status, nullptr);
}

hipError_t launch_time_dep(int Nlevel, int Ns, int k0, int k1, double* n, const double* nOld, const double* Gamma,
                           double dt, int* status, hipStream_t stream)
{
    if (Nlevel > 64)
        return hipErrorInvalidValue;
    const int tb = solve_block_threads(Nlevel);
    const size_t lds = solve_ws_doubles(Nlevel) * sizeof(double) * tb;
    hipError_t e = solve_set_lds((const void*)time_dep_kernel<false>, lds);
    if (e != hipSuccess)
        return e;
    LWHIP_LAUNCH(time_dep_kernel<false>, dim3((Ns + tb - 1) / tb), dim3(tb), lds, stream, Nlevel, Ns, k0, k1, n, nOld, Gamma,
                       dt, status, (const TimeDepArgs*)nullptr);
    return hipGetLastError();
}

// all solved atoms of nBatch columns: block size and LDS from the largest atom, as launch_stat_eq (so stat_eq_blocks counts
// the blocks per atom)
hipError_t launch_time_dep_list(const TimeDepArgs* list, int Ns, int Natoms, int maxNlevel, int nBatch, hipStream_t stream)
{
    if (maxNlevel > 64 || Natoms <= 0 || nBatch < 1 || !list)
        return hipErrorInvalidValue;
    const int tb = solve_block_threads(maxNlevel);
    const size_t lds = solve_ws_doubles(maxNlevel) * sizeof(double) * tb;
    hipError_t e = solve_set_lds((const void*)time_dep_kernel<true>, lds);
    if (e != hipSuccess)
        return e;
    LWHIP_LAUNCH(time_dep_kernel<true>, dim3((Ns + tb - 1) / tb, Natoms, nBatch), dim3(tb), lds, stream, 0, 0, 0, 0, (double*)nullptr,
                       (const double*)nullptr, (const double*)nullptr, 0.0, (int*)nullptr, list);
    return hipGetLastError();
}

// ---- nr_post_update_impl with F / Ftd: Source/UpdatePopulations.cpp:230-394 --------------------------------
// change: the column's [slots][gridDim.x][2] pairs (listed atom q reports into slot slots[q]), or null: nothing is reported and
// no barrier is met.  A point outside the depth range, or whose system is singular, keeps its n and ne.
DEVINL void nr_post_body(const NrArgs& a, double* change, const int32_t* slots)
{
    extern __shared__ double lds[];
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    const int Ns = a.Ns;
    const bool inRange = k >= a.k0 && k < a.k1;
    const int Neqn = a.Neqn;
    const SolveWs w(lds, Neqn, blockDim.x, threadIdx.x);
    const LdsVec& dF = w.A;
    const LdsVec& Fg = w.b;
    bool ok = false;
    double ne = 0.0;
    if (inRange)
    {
        for (int i = 0; i < Neqn; ++i)
        {
            Fg[i] = 0.0;
            for (int j = 0; j < Neqn; ++j)
                dF[i * Neqn + j] = 0.0;
        }
        const double theta = 1.0;
        ne = a.ne[k];
        Fg[Neqn - 1] = ne;
        int start = 0;
        for (int q = 0; q < a.Natoms; ++q)
        {
            const NrAtom at = a.atoms[q];
            const int Nl = at.Nlevel;
            const double* G = a.Gamma + at.gammaOff;
            const double* n = a.n + (size_t)at.levelOff * Ns;
            // F :230-257 / Ftd :259-292
            for (int l = 0; l < Nl; ++l)
            {
                double v = 0.0;
                if (a.timeDep)
                {
                    for (int ll = 0; ll < Nl; ++ll)
                        v += G[((size_t)l * Nl + ll) * Ns + k] * n[(size_t)ll * Ns + k];
                    v *= theta * a.dt;
                    v -= n[(size_t)l * Ns + k] - a.nPrev[(size_t)(at.eqOff + l) * Ns + k];
                }
                else
                {
                    for (int ll = 0; ll < Nl; ++ll)
                        v -= G[((size_t)l * Nl + ll) * Ns + k] * n[(size_t)ll * Ns + k];
                }
                Fg[start + l] = v;
            }
            double nTotCur = 0.0;
            for (int ll = 0; ll < Nl; ++ll)
                nTotCur += n[(size_t)ll * Ns + k];
            Fg[start + Nl - 1] = nTotCur - a.nTotal[(size_t)at.atom * Ns + k];
            double eleContrib = 0.0;
            for (int ll = 0; ll < Nl; ++ll)
                eleContrib += a.stages[at.eqOff + ll] * n[(size_t)ll * Ns + k];
            Fg[Neqn - 1] -= eleContrib;
            // Jacobian :322-372
            for (int l = 0; l < Nl; ++l)
                for (int ll = 0; ll < Nl; ++ll)
                    dF[(start + l) * Neqn + start + ll] = -G[((size_t)l * Nl + ll) * Ns + k];
            if (a.timeDep)
            {
                for (int l = 0; l < Nl; ++l)
                    for (int ll = 0; ll < Nl; ++ll)
                        dF[(start + l) * Neqn + start + ll] *= -theta * a.dt;
                for (int l = 0; l < Nl; ++l)
                    dF[(start + l) * Neqn + start + l] -= 1.0;
            }
            const double* Cm = a.Cmat + at.gammaOff;
            for (int tr = at.trBegin; tr < at.trEnd; ++tr)
            {
                if (a.transType[tr] != LWHIP_CONTINUUM)
                    continue;
                const int ti = a.transLi[tr], tj = a.transLj[tr];
                const double preconRji = G[((size_t)ti * Nl + tj) * Ns + k] - a.crsw * Cm[((size_t)ti * Nl + tj) * Ns + k];
                double entry = -(preconRji / ne) * n[(size_t)tj * Ns + k];
                if (a.timeDep)
                    entry *= -theta * a.dt;
                dF[(start + ti) * Neqn + Neqn - 1] += entry;
            }
            if (a.dC)
            {
                const double* dC = a.dC + (size_t)at.dcOff * Ns;
                for (int i = 0; i < Nl; ++i)
                {
                    double entry = 0.0;
                    for (int ll = 0; ll < Nl; ++ll)
                        entry -= dC[((size_t)i * Nl + ll) * Ns + k] * n[(size_t)ll * Ns + k];
                    if (a.timeDep)
                        entry *= -theta * a.dt;
                    dF[(start + i) * Neqn + Neqn - 1] += entry;
                }
            }
            for (int c = 0; c < Neqn; ++c)
                dF[(start + Nl - 1) * Neqn + c] = 0.0;
            for (int ll = 0; ll < Nl; ++ll)
            {
                dF[(start + Nl - 1) * Neqn + start + ll] = 1.0;
                dF[(Neqn - 1) * Neqn + start + ll] = -a.stages[at.eqOff + ll];
            }
            start += Nl;
        }
        Fg[Neqn - 1] -= a.backgroundNe[k];
        dF[(Neqn - 1) * Neqn + Neqn - 1] = 1.0;
        for (int i = 0; i < Neqn; ++i)
            Fg[i] *= -1.0;
        ok = d_solve_lin_eq(Neqn, w);
        if (!ok)
            atomicExch(a.status, LWHIP_ERR_SINGULAR);
    }
    // n += delta; per listed atom the change of what this thread wrote.  (The loop bounds are the block's; the thread's own
    // work hangs on `ok`.  Successive reports reuse report_change's shared arrays: a barrier between them.)
    int start = 0;
    for (int q = 0; q < a.Natoms; ++q)
    {
        const NrAtom at = a.atoms[q];
        double best = 0.0;
        int bestIdx = 0x7fffffff;
        if (ok)
        {
            double* n = a.n + (size_t)at.levelOff * Ns;
            for (int ll = 0; ll < at.Nlevel; ++ll)
            {
                const double old = n[(size_t)ll * Ns + k];
                const double cur = old + Fg[start + ll];
                n[(size_t)ll * Ns + k] = cur;
                if (cur != 0.0)
                {
                    const double change1 = fabs((cur - old) / cur);
                    if (change1 > best)
                    {
                        best = change1;
                        bestIdx = ll * Ns + k;
                    }
                }
            }
        }
        start += at.Nlevel;
        if (change)
        {
            report_change(best, bestIdx, change + (size_t)slots[q] * 2 * gridDim.x);
            __syncthreads();
        }
    }
    if (ok)
        a.ne[k] = ne + Fg[Neqn - 1];
}

// BATCH: column batches -- blockIdx.z picks the column's argument block (read through the constant address space)
template <bool BATCH> __global__ void nr_post_kernel(const NrArgs a0, const NrListArgs* __restrict__ list)
{
    dbg_poison_lds();
    if constexpr (BATCH)
    {
        const NrListArgs l = ld_c(CTAB(NrListArgs, list) + blockIdx.z);
        nr_post_body(l.a, l.change, l.slots);
    }
    else
        nr_post_body(a0, nullptr, nullptr);
}

int nr_post_blocks(int Ns, int Neqn)
{
    const int tb = solve_block_threads(Neqn);
    return (Ns + tb - 1) / tb;
}

// list: nBatch argument blocks on the device, `a` the first of them (its Neqn and Ns are every column's)
hipError_t launch_nr_post(const NrArgs& a, hipStream_t stream, const NrListArgs* list, int nBatch)
{
    if (a.Neqn > 64)
        return hipErrorInvalidValue;
    const int tb = solve_block_threads(a.Neqn);
    const size_t lds = solve_ws_doubles(a.Neqn) * sizeof(double) * tb;
    hipError_t e = solve_set_lds(list ? (const void*)nr_post_kernel<true> : (const void*)nr_post_kernel<false>, lds);
    if (e != hipSuccess)
        return e;
    if (list)
        LWHIP_LAUNCH(nr_post_kernel<true>, dim3((a.Ns + tb - 1) / tb, 1, nBatch > 0 ? nBatch : 1), dim3(tb), lds, stream, a, list);
    else
        LWHIP_LAUNCH(nr_post_kernel<false>, dim3((a.Ns + tb - 1) / tb), dim3(tb), lds, stream, a, list);
    return hipGetLastError();
}

// ---- Ng acceleration of the populations: Ng::accelerate + Ng::max_change (Source/Ng.hpp:52-156) of every active column in ONE
// launch.  A lone context is a batch of one column (lwhip_ng_configure); lwhip_batch_ng_configure brings n. ------------------
// One workgroup per (active column, solved atom); the column is picked through the compacted list as in batch_conv_kernel.
// All per-column state is on the device: the store slot, the accelerate decision and the slots of the earlier solutions are
// derived from the column's own count[col] and the three options, so columns on different schedules (one was inactive for some
// calls) share the launch and a call uploads nothing.
// The system of Norder x Norder weighted dot products can be ill conditioned, so every one of its No + No^2 sums is formed in
// the reference's order -- yet not all by a single lane: lane e < No + No^2 owns b(j) or A(i, j) and adds its terms for
// k = 0 .. L-1 in sequence; the workgroup stages weight(k) = 1 / |n[k]| and the No + 1 rows Delta(i, k) for NG_CHUNK values of k
// at a time through LDS (coalesced loads by all lanes; each Delta is one subtraction, formed once).  Contraction is off in this
// file: a term is two roundings of the products and the `+=` one more, as the reference's loop has them.  Rows are NG_CHUNK + 1
// doubles apart: the lanes of a sum read different rows at the same k, which would otherwise all sit in one bank pair.
// count[col] is read by every workgroup of the column and written once, by the workgroup that finishes last (a ticket per
// column): no workgroup can see the new count in the launch that made it.  With one solved atom the first workgroup is the last.
// tests/golden/ng_step_bits.json holds what a step leaves in n and reports, bit for bit.
enum { NG_CHUNK = 64, NG_ROW = NG_CHUNK + 1, NG_THREADS = 256 };
size_t ng_lds_bytes(int Norder)
{
    const int No = Norder > 0 ? Norder : 1;
    return (8 + (size_t)(No + 2) * NG_ROW + solve_ws_doubles(No)) * sizeof(double);
}

__global__ void __launch_bounds__(NG_THREADS) ng_kernel(const NgArgs a)
{
    dbg_poison_lds();
    extern __shared__ double lds[];
    __shared__ int sSlot[LWHIP_NG_MAX_ORDER + 2];
    __shared__ double sV[NG_THREADS / 64];
    __shared__ int sI[NG_THREADS / 64];
    const int col = a.cols ? a.cols[blockIdx.x] : (int)blockIdx.x;
    const NgAtom at = a.atoms[blockIdx.y];
    const NgCol cc = a.columns[col];
    const int L = at.len, No = a.Norder, nslots = No + 2;
    double* n = cc.n + (size_t)at.nOff;
    double* prev = a.history + (size_t)col * a.histStride + (size_t)at.histOff;
    auto slot = [&](int s) { return prev + (size_t)s * L; };
    // Ng::accelerate :52-65 for this column's own call count
    const int stored = a.count[col];
    const int storeSlot = stored % nslots; // :62
    const int count = stored + 1;
    const bool doAccel = No > 0 && count >= a.Ndelay && ((count - a.Ndelay) % a.Nperiod) == 0;
    if (threadIdx.x < nslots) // slots of count-1, count-2, ... count-Norder-2
        sSlot[threadIdx.x] = ((count - 1 - (int)threadIdx.x) % nslots + nslots) % nslots;
    for (int k = threadIdx.x; k < L; k += NG_THREADS)
        slot(storeSlot)[k] = n[k];
    __syncthreads();
    if (doAccel)
    {
        double* bco = lds;               // [No]
        double* rows = lds + 8;          // [No + 2][NG_ROW]: weight, Delta(0) .. Delta(No)
        const SolveWs w(rows + (size_t)(No + 2) * NG_ROW, No, 1, 0); // the solving lane's workspace
        const int e = threadIdx.x, nSums = No + No * No;
        // lane e: b(j) for e < No, else A(i, j) -- rows of Delta(j + 1) and Delta(i + 1)
        const int j = e < No ? e : (e - No) / No, i = e < No ? 0 : (e - No) % No;
        const double* rW = rows;
        const double* rD0 = rows + NG_ROW;
        const double* rDj = rows + (size_t)(j + 2) * NG_ROW;
        const double* rDi = rows + (size_t)(i + 2) * NG_ROW;
        double acc = 0.0;
        for (int k0 = 0; k0 < L; k0 += NG_CHUNK)
        {
            const int m = min((int)NG_CHUNK, L - k0);
            for (int q = threadIdx.x; q < nslots * NG_CHUNK; q += NG_THREADS)
            {
                const int r = q / NG_CHUNK, kk = q % NG_CHUNK;
                if (kk < m)
                {
                    const int k = k0 + kk;
                    rows[r * NG_ROW + kk] = r == 0 ? 1.0 / fabs(n[k]) : slot(sSlot[r - 1])[k] - slot(sSlot[r])[k];
                }
            }
            __syncthreads();
            if (e < No)
                for (int kk = 0; kk < m; ++kk)
                    acc += rW[kk] * rD0[kk] * (rD0[kk] - rDj[kk]);
            else if (e < nSums)
                for (int kk = 0; kk < m; ++kk)
                    acc += rW[kk] * (rDj[kk] - rD0[kk]) * (rDi[kk] - rD0[kk]);
            __syncthreads();
        }
        if (e < No)
            w.b[j] = acc;
        else if (e < nSums)
            w.A[i * No + j] = acc;
        __syncthreads();
        if (threadIdx.x == 0)
        {
            const bool ok = d_solve_lin_eq(No, w);
            for (int q = 0; q < No; ++q)
                bco[q] = ok ? (double)w.b[q] : 0.0;
            if (!ok)
                atomicExch(cc.status, LWHIP_ERR_SINGULAR);
        }
        __syncthreads();
        // sol += sum_i b_i (previous(count-i-2) - previous(count-1)), then previous(count-1) = sol  :104-113
        double* p0 = slot(sSlot[0]);
        for (int k = threadIdx.x; k < L; k += NG_THREADS)
        {
            double v = n[k];
            const double p0k = p0[k];
            for (int q = 0; q < No; ++q)
                v += bco[q] * (slot(sSlot[q + 1])[k] - p0k);
            n[k] = v;
        }
        __syncthreads();
        for (int k = threadIdx.x; k < L; k += NG_THREADS)
            p0[k] = n[k];
        __syncthreads();
    }
    // max_change :138-156 between the last two stored solutions (count >= 2 here: configure stored the first)
    double best = 0.0;
    int bestIdx = 0x7fffffff;
    {
        const double* old = slot(sSlot[1]);
        const double* cur = slot(storeSlot);
        for (int k = threadIdx.x; k < L; k += NG_THREADS)
        {
            const double c = cur[k];
            if (c != 0.0)
            {
                const double change = fabs((c - old[k]) / c);
                if (change > best)
                {
                    best = change;
                    bestIdx = k;
                }
            }
        }
    }
    // (the largest value, the first index among equal values: the rule does not depend on the order of combination)
    for (int s = 32; s > 0; s >>= 1)
    {
        const double ov = __shfl_xor(best, s);
        const int oi = __shfl_xor(bestIdx, s);
        if (ov > best || (ov == best && oi < bestIdx))
        {
            best = ov;
            bestIdx = oi;
        }
    }
    if ((threadIdx.x & 63) == 0)
    {
        sV[threadIdx.x >> 6] = best;
        sI[threadIdx.x >> 6] = bestIdx;
    }
    __syncthreads(); // (also: every lane's read of count[col] lies before the ticket below)
    if (threadIdx.x == 0)
    {
        for (int q = 1; q < NG_THREADS / 64; ++q)
            if (sV[q] > best || (sV[q] == best && sI[q] < bestIdx))
            {
                best = sV[q];
                bestIdx = sI[q];
            }
        double* ch = a.change + ((size_t)col * a.Natoms + blockIdx.y) * 2;
        ch[0] = best;
        ch[1] = best > 0.0 ? (double)bestIdx : 0.0;
        // the column's last workgroup writes count + 1 back, after every workgroup's read of it
        __threadfence();
        if (atomicAdd(a.ticket + col, 1) == (int)gridDim.y - 1)
        {
            a.ticket[col] = 0;
            a.accel[col] = doAccel ? 1 : 0;
            a.count[col] = count;
        }
    }
}

// ng_configure: every column's current populations into slot 0, the other slots cleared, count = 1 -- one launch,
// one workgroup per (column, solved atom), ALL columns
__global__ void __launch_bounds__(NG_THREADS) ng_seed_kernel(const NgArgs a)
{
    const int col = blockIdx.x;
    const NgAtom at = a.atoms[blockIdx.y];
    const double* n = a.columns[col].n + (size_t)at.nOff;
    double* prev = a.history + (size_t)col * a.histStride + (size_t)at.histOff;
    const int L = at.len;
    for (int k = threadIdx.x; k < L; k += NG_THREADS)
        prev[k] = n[k];
    for (size_t k = (size_t)L + threadIdx.x; k < (size_t)(a.Norder + 2) * L; k += NG_THREADS)
        prev[k] = 0.0;
    if (blockIdx.y == 0 && threadIdx.x == 0)
    {
        a.count[col] = 1; // the constructor stores the current solution, Ng.hpp:34-38
        a.accel[col] = 0;
        a.ticket[col] = 0;
    }
}

hipError_t launch_ng(const NgArgs& a, int nActive, hipStream_t stream)
{
    if (nActive < 1 || a.Natoms < 1 || a.Norder < 0 || a.Norder > LWHIP_NG_MAX_ORDER || (a.Norder > 0 && a.Nperiod < 1))
        return hipErrorInvalidValue;
    LWHIP_LAUNCH(ng_kernel, dim3(nActive, a.Natoms), dim3(NG_THREADS), ng_lds_bytes(a.Norder), stream, a);
    return hipGetLastError();
}

hipError_t launch_ng_seed(const NgArgs& a, int n, hipStream_t stream)
{
    if (n < 1 || a.Natoms < 1)
        return hipErrorInvalidValue;
    LWHIP_LAUNCH(ng_seed_kernel, dim3(n, a.Natoms), dim3(NG_THREADS), 0, stream, a);
    return hipGetLastError();
}
}
