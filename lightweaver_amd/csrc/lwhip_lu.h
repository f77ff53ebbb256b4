// lwhip_lu.h -- the reference's dense solver with the system in registers: solve_lin_eq (Source/LuSolve.cpp:8-132), Crout LU
// with implicit row scaling, partial pivoting and one residual-correction pass.  Used by the population updates
// (lwhip_pops.hip, N <= 6) and by the 4 x 4 DELO-Bezier3 step of the Stokes march (lwhip_stokes_fs.hip).  Both units include it
// after `#pragma clang fp contract(off)`, so that its operations match the reference's one for one.
#pragma once
#include "lwhip_device.h"

namespace lwhip
{
// The same solver with the system in REGISTERS, for the small level counts (N <= 6: H and Ca II of the benchmark): every
// loop is unrolled, the dynamically indexed accesses of the pivoting (row iMax, x[index[i]]) become selects over the
// rows.  Operation for operation d_solve_lin_eq of lwhip_pops.hip (each element's sums are formed in the same order), so the results
// are the same bits; what changes is the latency: an LDS round trip per matrix element made the 6 x 6 solve of one
// depth point ~25 us, here it is a straight-line stream of ~1 500 instructions.
template <int N> DEVINL bool d_solve_lin_eq_reg(double (&A)[N][N], double (&b)[N])
{
    double A0[N][N], b0[N], vv[N], res[N];
    int index[N];
#pragma unroll
    for (int i = 0; i < N; ++i)
    {
        b0[i] = b[i];
#pragma unroll
        for (int j = 0; j < N; ++j)
            A0[i][j] = A[i][j];
    }
    // lu_decompose :8-70
    bool singular = false;
#pragma unroll
    for (int i = 0; i < N; ++i)
    {
        double big = 0.0;
#pragma unroll
        for (int j = 0; j < N; ++j)
            big = fmax(big, fabs(A[i][j]));
        if (big == 0.0)
            singular = true;
        vv[i] = 1.0 / big;
    }
    if (singular)
        return false;
#pragma unroll
    for (int j = 0; j < N; ++j)
    {
#pragma unroll
        for (int i = 0; i < j; ++i)
        {
            double sum = A[i][j];
#pragma unroll
            for (int q = 0; q < i; ++q)
                sum -= A[i][q] * A[q][j];
            A[i][j] = sum;
        }
        int iMax = 0;
        double big = 0.0;
#pragma unroll
        for (int i = j; i < N; ++i)
        {
            double sum = A[i][j];
#pragma unroll
            for (int q = 0; q < j; ++q)
                sum -= A[i][q] * A[q][j];
            A[i][j] = sum;
            const double cand = vv[i] * fabs(sum);
            if (big < cand)
            {
                iMax = i;
                big = cand;
            }
        }
        // rows j and iMax change places (iMax stays 0 when no candidate is positive: the reference then swaps with row 0)
#pragma unroll
        for (int r = 0; r < N; ++r)
        {
            if (r == j)
                continue;
            const bool sw = iMax == r;
#pragma unroll
            for (int q = 0; q < N; ++q)
            {
                const double ar = A[r][q], aj = A[j][q];
                A[r][q] = sw ? aj : ar;
                A[j][q] = sw ? ar : aj;
            }
            vv[r] = sw ? vv[j] : vv[r];
        }
        index[j] = iMax;
        if (A[j][j] == 0.0)
            A[j][j] = 1e-20;
        const double tmp = 1.0 / A[j][j];
#pragma unroll
        for (int i = j + 1; i < N; ++i)
            A[i][j] *= tmp;
    }
    // lu_backsub :72-101
    auto backsub = [&](double (&x)[N]) {
        int ii = -1;
#pragma unroll
        for (int i = 0; i < N; ++i)
        {
            const int ip = index[i];
            double sum = x[i];
#pragma unroll
            for (int r = 0; r < N; ++r)
                sum = (ip == r) ? x[r] : sum;
            const double xi = x[i];
#pragma unroll
            for (int r = 0; r < N; ++r)
                x[r] = (ip == r) ? xi : x[r];
            if (ii >= 0)
            {
#pragma unroll
                for (int j = 0; j < i; ++j)
                    if (j >= ii)
                        sum -= A[i][j] * x[j];
            }
            else if (sum != 0.0)
                ii = i;
            x[i] = sum;
        }
#pragma unroll
        for (int i = N - 1; i >= 0; --i)
        {
            double sum = x[i];
#pragma unroll
            for (int j = i + 1; j < N; ++j)
                sum -= A[i][j] * x[j];
            x[i] = sum / A[i][i];
        }
    };
    backsub(b);
    // one pass of iterative improvement :114-131
#pragma unroll
    for (int i = 0; i < N; ++i)
    {
        double r = b0[i];
#pragma unroll
        for (int j = 0; j < N; ++j)
            r -= A0[i][j] * b[j];
        res[i] = r;
    }
    backsub(res);
#pragma unroll
    for (int i = 0; i < N; ++i)
        b[i] += res[i];
    return true;
}
}
