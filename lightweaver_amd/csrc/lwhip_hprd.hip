// lwhip_hprd.hip -- the hybrid-PRD interpolation tables built on the device: lwhip_hprd_build / lwhip_hprd_free.
//
// What configure_hprd_coeffs (Source/Prd.cpp:697-946) leaves in the reference's Context -- the wavelengths where a PRD line
// is active (prdIdxs), those that scatter into them under the atmosphere's line-of-sight velocities (hPrdIdxs), the
// (row of JRest, weight) list of every (such wavelength, ray, direction, depth) (JCoeffs) and every PRD line's rho
// interpolation table (hPrdCoeffs) -- as the flat lwhip_hprd that lwhip_options.hprd takes.  Every cell is independent and
// needs only multiply, divide, add and compare in fp64, all correctly rounded on the device: the tables are the reference's
// bit for bit.  The specification is the restatement oracle/lw_oracle.c::lworacle_hprd_build, which the tests pin to the core.
//
// One thread per cell, depth fastest (consecutive lanes read consecutive vlosMu):
//   hprd_flag_kernel     one workgroup per wavelength: does any (mu, toObs, k) walk reach a PRD-active wavelength? (:765-811)
//                        The flags go to the host, which forms hPrdIdxs -- the layout of everything below depends on it.
//   hprd_jcoeff_kernel   <false>: the length of every cell's list into jCoeffOff; <true>: the same walk again, writing the
//                        entries at the cell's offset (:816-897).  Between the two an exclusive scan of the lengths on the
//                        device (hprd_scan_*: tile sums, one workgroup over the sums, tiles again); only the 8-byte total
//                        reaches the host, to size the entry buffer.
//   hprd_rho_kernel      per (PRD line, lt, mu, toObs, k): the two clamped ends, else upper_bound - 1 by bisection (:899-939).
// LDS: the four wavefront totals of a workgroup scan (32 bytes); the flag reduction is __syncthreads_or.
#include "lwhip_host.h"
#include "lwhip_device.h"

// No fused multiply-adds: the operations match the reference's one for one (fac = 1.0 + (v * s) / c, lambda * fac, the
// differences and the quotient of a weight are each rounded once).  No fast-math anywhere in the library's flags.
#pragma clang fp contract(off)

#include <cstring>
#include <vector>

namespace lwhip
{
namespace
{
enum { HPRD_THREADS = 256, HPRD_SCAN_ITEMS = 4, HPRD_SCAN_TILE = HPRD_THREADS * HPRD_SCAN_ITEMS };
constexpr uint64_t HPRD_MAGIC = 0x6c77686970485052ull; // "lwhipHPR": lwhip_hprd_free frees only what lwhip_hprd_build made

struct HprdIn
{
    const double* wl;      // [Nspect] the global wavelength grid
    const double* vlos;    // [Nrays, Ns] vlosMu
    const int32_t* la2prd; // [Nspect] row of JRest of a PRD-active wavelength, -1 elsewhere (prdActive and la_to_prdLa in one)
    int32_t Nspect, Nrays, Ns;
};
struct HprdLine
{
    int64_t cellOff; // first cell (lt, mu, toObs, k) of the line in the flat rho table
    int32_t waveOff; // the line's own grid in lineWave
    int32_t nlt;
};

// fac of a cell: 1.0 + vlosMu(mu, k) * sign / CLight, in the reference's order
__device__ __forceinline__ double hprd_fac(const HprdIn& a, int mu, int toObs, int k)
{
    const double sgn = toObs ? 1.0 : -1.0;
    return 1.0 + a.vlos[(size_t)mu * a.Ns + k] * sgn / CLight;
}

__global__ __launch_bounds__(HPRD_THREADS) void hprd_flag_kernel(HprdIn a, int32_t* __restrict__ flags)
{
    const int la = blockIdx.x, Nspect = a.Nspect;
    const int prevIndex = la - 1 > 0 ? la - 1 : 0;
    const int nextIndex = la + 1 < Nspect - 1 ? la + 1 : Nspect - 1;
    const double wPrev = a.wl[prevIndex], wNext = a.wl[nextIndex];
    const int ncell = a.Nrays * 2 * a.Ns;
    int hit = 0;
    for (int c = threadIdx.x; c < ncell && !hit; c += HPRD_THREADS)
    {
        const int k = c % a.Ns, r = c / a.Ns;
        const double fac = hprd_fac(a, r >> 1, r & 1, k);
        const double prevLambda = wPrev * fac;
        const double nextLambda = wNext * fac;
        int i = la;
        for (; a.wl[i] > prevLambda && i > 0; --i)
            ;
        for (; i < Nspect; ++i)
        {
            if (a.la2prd[i] >= 0)
            {
                hit = 1;
                break;
            }
            else if (a.wl[i] > nextLambda)
                break;
        }
    }
    hit = __syncthreads_or(hit);
    if (threadIdx.x == 0)
        flags[la] = hit;
}

// The list of one cell (:816-897).  FILL = false counts; FILL = true writes at most `cap` entries (the count of the first
// pass: the same walk on the same inputs gives the same number, the bound only keeps a store inside the buffer whatever).
template <bool FILL>
__device__ __forceinline__ int hprd_jcoeff_cell(const HprdIn& a, int idx, double fac, lwhip_j_coeff* __restrict__ out, int64_t cap)
{
    const int Nspect = a.Nspect;
    const double* __restrict__ wl = a.wl;
    const int32_t* __restrict__ la2prd = a.la2prd;
    int n = 0;
    auto push = [&](int row, double frac) {
        if (FILL && n < cap)
        {
            lwhip_j_coeff e;
            e.frac = frac;
            e.idx = row;
            e._pad = 0;
            out[n] = e;
        }
        ++n;
    };
    const int prevIndex = idx - 1 > 0 ? idx - 1 : 0;
    const int nextIndex = idx + 1 < Nspect - 1 ? idx + 1 : Nspect - 1;
    const double prevLambda = wl[prevIndex] * fac;
    const double lambdaRest = wl[idx] * fac;
    const double nextLambda = wl[nextIndex] * fac;
    bool doLowerHalf = true, doUpperHalf = true;
    if (prevIndex == idx)
    {
        // the blue end of the grid: constant extrapolation
        doLowerHalf = false;
        for (int i = 0; i < Nspect; ++i)
        {
            if (wl[i] <= lambdaRest && la2prd[i] >= 0)
                push(la2prd[i], 1.0);
            else
                break;
        }
    }
    else if (nextIndex == idx)
    {
        // the red end, in decreasing i
        doUpperHalf = false;
        for (int i = Nspect - 1; i >= 0; --i)
        {
            if (wl[i] > lambdaRest && la2prd[i] >= 0)
                push(la2prd[i], 1.0);
            else
                break;
        }
    }
    int i = idx;
    // (the reference tests wavelength(i) before i >= 0, :872, and reads before the array at i = -1; the walk starts at 0 either way)
    for (; i >= 0 && wl[i] > prevLambda; --i)
        ;
    if (i < 0)
        i = 0;
    for (; i < Nspect; ++i)
    {
        const double lambdaI = wl[i];
        if (lambdaI > nextLambda)
            break;
        const int row = la2prd[i];
        if (doLowerHalf && row >= 0 && lambdaI > prevLambda && lambdaI <= lambdaRest)
        {
            const double frac = (lambdaI - prevLambda) / (lambdaRest - prevLambda);
            push(row, frac);
        }
        else if (doUpperHalf && row >= 0 && lambdaI > lambdaRest && lambdaI < nextLambda)
        {
            const double frac = (lambdaI - lambdaRest) / (nextLambda - lambdaRest);
            push(row, 1.0 - frac);
        }
    }
    return n;
}

// cell = ((hq * Nrays + mu) * 2 + toObs) * Ns + k.  FILL = false: off[cell] <- length; FILL = true: off holds the offsets.
template <bool FILL>
__global__ __launch_bounds__(HPRD_THREADS) void hprd_jcoeff_kernel(HprdIn a, const int32_t* __restrict__ hIdx, int64_t ncell,
                                                                   int64_t* __restrict__ off, lwhip_j_coeff* __restrict__ jc)
{
    const int64_t cell = (int64_t)blockIdx.x * HPRD_THREADS + threadIdx.x;
    if (cell >= ncell)
        return;
    const int k = (int)(cell % a.Ns);
    const int64_t r = cell / a.Ns;
    const int toObs = (int)(r & 1);
    const int mu = (int)((r >> 1) % a.Nrays);
    const int hq = (int)((r >> 1) / a.Nrays);
    const double fac = hprd_fac(a, mu, toObs, k);
    if (FILL)
    {
        const int64_t base = off[cell];
        (void)hprd_jcoeff_cell<true>(a, hIdx[hq], fac, jc + base, off[cell + 1] - base);
    }
    else
        off[cell] = hprd_jcoeff_cell<false>(a, hIdx[hq], fac, nullptr, 0);
}

// exclusive scan of one value per thread over the workgroup (4 wavefronts of 64); *total: the workgroup's sum, in every thread
__device__ __forceinline__ int64_t hprd_block_scan(int64_t x, int64_t* total)
{
    __shared__ int64_t waveSum[HPRD_THREADS / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int64_t inc = x;
    for (int d = 1; d < 64; d <<= 1)
    {
        const int64_t y = __shfl_up(inc, d, 64);
        if (lane >= d)
            inc += y;
    }
    if (lane == 63)
        waveSum[w] = inc;
    __syncthreads();
    int64_t base = 0, tot = 0;
    for (int i = 0; i < HPRD_THREADS / 64; ++i)
    {
        const int64_t s = waveSum[i];
        base += i < w ? s : 0;
        tot += s;
    }
    __syncthreads(); // (waveSum is written again by the caller's next round)
    *total = tot;
    return base + inc - x;
}

// x[0, n) in tiles of HPRD_SCAN_TILE: the sum of every tile
__global__ __launch_bounds__(HPRD_THREADS) void hprd_scan_sums_kernel(const int64_t* __restrict__ x, int64_t n, int64_t* __restrict__ tileSum)
{
    const int64_t first = (int64_t)blockIdx.x * HPRD_SCAN_TILE + (int64_t)threadIdx.x * HPRD_SCAN_ITEMS;
    int64_t s = 0;
    for (int j = 0; j < HPRD_SCAN_ITEMS; ++j)
        s += first + j < n ? x[first + j] : 0;
    int64_t tot;
    (void)hprd_block_scan(s, &tot);
    if (threadIdx.x == 0)
        tileSum[blockIdx.x] = tot;
}
// one workgroup: the tile sums to their exclusive prefix, the grand total to *total
__global__ __launch_bounds__(HPRD_THREADS) void hprd_scan_top_kernel(int64_t* __restrict__ tileSum, int64_t nTiles, int64_t* __restrict__ total)
{
    int64_t carry = 0;
    for (int64_t b = 0; b < nTiles; b += HPRD_THREADS)
    {
        const int64_t i = b + threadIdx.x;
        const int64_t x = i < nTiles ? tileSum[i] : 0;
        int64_t tot;
        const int64_t ex = hprd_block_scan(x, &tot);
        if (i < nTiles)
            tileSum[i] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0)
        *total = carry;
}
// x <- its exclusive prefix, given the prefix of the tiles
__global__ __launch_bounds__(HPRD_THREADS) void hprd_scan_apply_kernel(int64_t* __restrict__ x, int64_t n, const int64_t* __restrict__ tileSum)
{
    const int64_t first = (int64_t)blockIdx.x * HPRD_SCAN_TILE + (int64_t)threadIdx.x * HPRD_SCAN_ITEMS;
    int64_t v[HPRD_SCAN_ITEMS], s = 0;
    for (int j = 0; j < HPRD_SCAN_ITEMS; ++j)
    {
        v[j] = first + j < n ? x[first + j] : 0;
        s += v[j];
    }
    int64_t tot;
    int64_t run = tileSum[blockIdx.x] + hprd_block_scan(s, &tot);
    for (int j = 0; j < HPRD_SCAN_ITEMS; ++j)
    {
        if (first + j < n)
            x[first + j] = run;
        run += v[j];
    }
}

__global__ __launch_bounds__(HPRD_THREADS) void hprd_rho_kernel(HprdIn a, const double* __restrict__ lineWave, const HprdLine* __restrict__ lines,
                                                                int Nlines, int64_t ncell, lwhip_rho_coeff* __restrict__ out)
{
    const int64_t cell = (int64_t)blockIdx.x * HPRD_THREADS + threadIdx.x;
    if (cell >= ncell)
        return;
    int q = 0;
    while (q + 1 < Nlines && cell >= lines[q + 1].cellOff)
        ++q;
    const HprdLine L = lines[q];
    const int64_t local = cell - L.cellOff;
    const int k = (int)(local % a.Ns);
    const int64_t r = local / a.Ns;
    const int toObs = (int)(r & 1);
    const int mu = (int)((r >> 1) % a.Nrays);
    const int lt = (int)((r >> 1) / a.Nrays);
    const double* __restrict__ w = lineWave + L.waveOff;
    const int nlt = L.nlt;
    const double lambdaRest = w[lt] * hprd_fac(a, mu, toObs, k);
    int i0, i1;
    double frac;
    d_hprd_rho_coeff(w, nlt, lambdaRest, i0, i1, frac);
    lwhip_rho_coeff c;
    c.frac = frac;
    c.i0 = i0;
    c.i1 = i1;
    out[cell] = c;
}

// what lwhip_hprd_build hands out: the descriptor first, then what owns its arrays
struct HprdOwned
{
    lwhip_hprd h{};
    uint64_t magic = HPRD_MAGIC;
    std::vector<int32_t> prdIdxs, hPrdIdxs, lineAtom, lineTrans;
    std::vector<const lwhip_rho_coeff*> rhoPtrs;
    double* JRest = nullptr;
    int64_t* off = nullptr;
    lwhip_j_coeff* jc = nullptr;
    lwhip_rho_coeff* rho = nullptr;
    ~HprdOwned()
    {
        std::free(JRest);
        std::free(off);
        std::free(jc);
        std::free(rho);
    }
};

// LWHIP_HPRD_TIMING=1: where the time of a build goes (a stream wait after every phase; tools/hprd_build_time.py reads it)
struct PhaseClock
{
    bool on;
    hipStream_t stream;
    std::chrono::steady_clock::time_point prev = std::chrono::steady_clock::now();
    void operator()(const char* what)
    {
        if (!on)
            return;
        (void)hipStreamSynchronize(stream);
        const auto now = std::chrono::steady_clock::now();
        std::fprintf(stderr, "  lwhip_hprd_build: %-10s %.3f ms\n", what, std::chrono::duration<double, std::milli>(now - prev).count());
        prev = now;
    }
};

unsigned grid_for(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

// Everything that touches the device.  `o` holds the line list, prdIdxs and the zeroed JRest already.
int hprd_build_device(const lwhip_problem& p, const std::vector<int32_t>& la2prd, const std::vector<HprdLine>& lines,
                      const std::vector<double>& lineWave, int64_t nRho, hipStream_t stream, HprdOwned& o)
{
    const int Nspect = p.Nlambda, Nrays = p.Nrays, Ns = p.Nspace, Nl = (int)lines.size();
    PhaseClock tick{ std::getenv("LWHIP_HPRD_TIMING") != nullptr, stream };
    DevMem m;
    m.stream = stream;
    // ---- one upload: [wavelength | vlosMu | the lines' grids | line records | la2prd] --------------------------------------
    const size_t oWl = 0, oV = oWl + Nspect, oLw = oV + (size_t)Nrays * Ns, oLine = oLw + lineWave.size(),
                 oLa = oLine + 2 * (size_t)Nl, nIn = oLa + ((size_t)Nspect + 1) / 2;
    static_assert(sizeof(HprdLine) == 2 * sizeof(double), "HprdLine is two doubles of the upload");
    std::vector<double> in(nIn, 0.0);
    std::memcpy(&in[oWl], p.wavelength, sizeof(double) * Nspect);
    std::memcpy(&in[oV], p.vlosMu, sizeof(double) * Nrays * Ns);
    std::memcpy(&in[oLw], lineWave.data(), sizeof(double) * lineWave.size());
    std::memcpy(&in[oLine], lines.data(), sizeof(HprdLine) * Nl);
    std::memcpy(&in[oLa], la2prd.data(), sizeof(int32_t) * Nspect);
    DevBuf<double> dIn;
    HIP_TRY(dIn.alloc(m, nIn, false));
    HIP_TRY(m.h2d(dIn.p, in.data(), nIn * sizeof(double))); // (`in` lives until the last wait below)
    HprdIn a;
    a.wl = dIn.p + oWl;
    a.vlos = dIn.p + oV;
    a.la2prd = (const int32_t*)(dIn.p + oLa);
    a.Nspect = Nspect;
    a.Nrays = Nrays;
    a.Ns = Ns;
    tick("upload");
    // ---- which wavelengths scatter into the PRD region: the flags come back, the host lays out the rest ----------------------
    DevBuf<int32_t> dFlags;
    HIP_TRY(dFlags.alloc(m, Nspect, false));
    LWHIP_LAUNCH(hprd_flag_kernel, dim3((unsigned)Nspect), dim3(HPRD_THREADS), 0, stream, a, dFlags.p);
    HIP_TRY(hipGetLastError());
    tick("flags");
    std::vector<int32_t> flags(Nspect);
    HIP_TRY(hipMemcpyAsync(flags.data(), dFlags.p, sizeof(int32_t) * Nspect, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    for (int la = 0; la < Nspect; ++la)
        if (flags[la])
            o.hPrdIdxs.push_back(la);
    const int NhPrd = (int)o.hPrdIdxs.size();
    o.hPrdIdxs.resize(std::max(NhPrd, 1), 0); // (never a null pointer in the descriptor)
    tick("flags d2h");
    // ---- JCoeffs: count, scan, (the total to the host), fill; the rho tables in between -----------------------------------------
    const int64_t ncell = (int64_t)NhPrd * Nrays * 2 * Ns;
    const int64_t nTiles = (ncell + HPRD_SCAN_TILE - 1) / HPRD_SCAN_TILE;
    if (ncell / HPRD_THREADS >= 0x7fffffff || nRho / HPRD_THREADS >= 0x7fffffff)
        return fail(LWHIP_ERR_UNSUPPORTED, "lwhip_hprd_build: more cells than one launch takes");
    DevBuf<int32_t> dHIdx;
    DevBuf<int64_t> dOff, dTile;
    DevBuf<lwhip_j_coeff> dJc;
    DevBuf<lwhip_rho_coeff> dRho;
    int64_t nj = 0;
    HIP_TRY(dOff.alloc(m, (size_t)ncell + 1, false));
    if (ncell > 0)
    {
        HIP_TRY(dHIdx.alloc(m, NhPrd, false));
        HIP_TRY(m.h2d(dHIdx.p, o.hPrdIdxs.data(), sizeof(int32_t) * NhPrd));
        HIP_TRY(dTile.alloc(m, (size_t)nTiles, false));
        LWHIP_LAUNCH(hprd_jcoeff_kernel<false>, dim3(grid_for(ncell, HPRD_THREADS)), dim3(HPRD_THREADS), 0, stream, a, dHIdx.p, ncell,
                     dOff.p, (lwhip_j_coeff*)nullptr);
        HIP_TRY(hipGetLastError());
        tick("count");
        LWHIP_LAUNCH(hprd_scan_sums_kernel, dim3((unsigned)nTiles), dim3(HPRD_THREADS), 0, stream, dOff.p, ncell, dTile.p);
        LWHIP_LAUNCH(hprd_scan_top_kernel, dim3(1), dim3(HPRD_THREADS), 0, stream, dTile.p, nTiles, dOff.p + ncell);
        LWHIP_LAUNCH(hprd_scan_apply_kernel, dim3((unsigned)nTiles), dim3(HPRD_THREADS), 0, stream, dOff.p, ncell, dTile.p);
        HIP_TRY(hipGetLastError());
        tick("scan");
    }
    else
        HIP_TRY(hipMemsetAsync(dOff.p, 0, sizeof(int64_t), stream));
    HIP_TRY(dRho.alloc(m, (size_t)nRho, false));
    LWHIP_LAUNCH(hprd_rho_kernel, dim3(grid_for(nRho, HPRD_THREADS)), dim3(HPRD_THREADS), 0, stream, a, dIn.p + oLw,
                 (const HprdLine*)(dIn.p + oLine), Nl, nRho, dRho.p);
    HIP_TRY(hipGetLastError());
    tick("rho");
    HIP_TRY(hipMemcpyAsync(&nj, dOff.p + ncell, sizeof(int64_t), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (nj < 0)
        return fail(LWHIP_ERR_DEVICE, "lwhip_hprd_build: negative JCoeffs total");
    tick("total d2h");
    HIP_TRY(dJc.alloc(m, (size_t)std::max<int64_t>(nj, 1), false));
    if (nj > 0)
    {
        LWHIP_LAUNCH(hprd_jcoeff_kernel<true>, dim3(grid_for(ncell, HPRD_THREADS)), dim3(HPRD_THREADS), 0, stream, a, dHIdx.p, ncell, dOff.p,
                     dJc.p);
        HIP_TRY(hipGetLastError());
    }
    tick("fill");
    // ---- the tables to the host, one wait ------------------------------------------------------------------------------------------
    o.off = (int64_t*)std::malloc(sizeof(int64_t) * ((size_t)ncell + 1));
    o.jc = (lwhip_j_coeff*)std::calloc((size_t)std::max<int64_t>(nj, 1), sizeof(lwhip_j_coeff));
    o.rho = (lwhip_rho_coeff*)std::malloc(sizeof(lwhip_rho_coeff) * (size_t)nRho);
    if (!o.off || !o.jc || !o.rho)
        return fail(LWHIP_ERR_INVALID, "lwhip_hprd_build: out of host memory");
    HIP_TRY(hipMemcpyAsync(o.off, dOff.p, sizeof(int64_t) * ((size_t)ncell + 1), hipMemcpyDeviceToHost, stream));
    if (nj > 0)
        HIP_TRY(hipMemcpyAsync(o.jc, dJc.p, sizeof(lwhip_j_coeff) * (size_t)nj, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(o.rho, dRho.p, sizeof(lwhip_rho_coeff) * (size_t)nRho, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    tick("tables d2h");
    o.h.NhPrd = NhPrd;
    return LWHIP_OK;
}
} // namespace
} // namespace lwhip

using namespace lwhip;

int lwhip_hprd_build(const lwhip_problem* prob, const lwhip_options* opts, int includeDetailed, lwhip_hprd** out)
{
    if (!out)
        return fail(LWHIP_ERR_INVALID, "lwhip_hprd_build: null out pointer");
    *out = nullptr;
    if (!prob)
        return fail(LWHIP_ERR_INVALID, "lwhip_hprd_build: null problem");
    const lwhip_problem& p = *prob;
    if (p.abiVersion != LWHIP_ABI_VERSION)
        return fail(LWHIP_ERR_INVALID, "lwhip_hprd_build: ABI version mismatch");
    if (p.grid2d)
        return fail(LWHIP_ERR_UNSUPPORTED, "lwhip_hprd_build: hybrid PRD: 1D contexts only");
    if (p.Nspace < 1 || p.Nrays < 1 || p.Nlambda < 1 || p.Natom < 0 || (p.Natom > 0 && !p.atoms))
        return fail(LWHIP_ERR_INVALID, "lwhip_hprd_build: need Nspace >= 1, Nrays >= 1, Nlambda >= 1 and the atoms");
    if (!p.vlosMu)
        return fail(LWHIP_ERR_INVALID, "lwhip_hprd_build: the problem has no vlosMu");
    if (!p.wavelength)
        return fail(LWHIP_ERR_INVALID, "lwhip_hprd_build: the problem has no wavelength grid");
    // the PRD lines: active atoms first, then -- on request -- the detailed ones (:712-735)
    auto o = std::make_unique<HprdOwned>();
    for (int pass = 0; pass < (includeDetailed ? 2 : 1); ++pass)
        for (int ia = 0; ia < p.Natom; ++ia)
        {
            const lwhip_atom& at = p.atoms[ia];
            if ((at.detailed != 0) != (pass == 1))
                continue;
            if (at.Ntrans > 0 && !at.trans)
                return fail(LWHIP_ERR_INVALID, "lwhip_hprd_build: an atom without its transitions");
            for (int kr = 0; kr < at.Ntrans; ++kr)
                if (at.trans[kr].type == LWHIP_LINE && at.trans[kr].prd && at.trans[kr].rhoPrd)
                {
                    o->lineAtom.push_back(ia);
                    o->lineTrans.push_back(kr);
                }
        }
    const int Nl = (int)o->lineAtom.size();
    const int Nspect = p.Nlambda, Ns = p.Nspace, Nrays = p.Nrays;
    std::vector<HprdLine> lines(Nl);
    std::vector<double> lineWave;
    int64_t nRho = 0;
    for (int q = 0; q < Nl; ++q)
    {
        const lwhip_transition& t = p.atoms[o->lineAtom[q]].trans[o->lineTrans[q]];
        const int nlt = t.Nred - t.Nblue;
        if (nlt < 2)
            return fail(LWHIP_ERR_INVALID, "lwhip_hprd_build: a PRD line with fewer than 2 wavelengths");
        if (t.Nblue < 0 || t.Nred > Nspect || !t.wavelength)
            return fail(LWHIP_ERR_INVALID, "lwhip_hprd_build: a PRD line outside the wavelength grid, or without its own grid");
        lines[q].cellOff = nRho;
        lines[q].waveOff = (int32_t)lineWave.size();
        lines[q].nlt = nlt;
        lineWave.insert(lineWave.end(), t.wavelength, t.wavelength + nlt);
        nRho += (int64_t)nlt * Nrays * 2 * Ns;
    }
    if (Nl == 0)
        return LWHIP_OK; // (the reference returns early and stays plain PRD)
    // wavelengths where a PRD line is active (:740-757)
    std::vector<int32_t> la2prd(Nspect, -1);
    for (int q = 0; q < Nl; ++q)
    {
        const lwhip_transition& t = p.atoms[o->lineAtom[q]].trans[o->lineTrans[q]];
        for (int la = t.Nblue; la < t.Nred; ++la)
            la2prd[la] = 0;
    }
    for (int la = 0; la < Nspect; ++la)
        if (la2prd[la] == 0)
        {
            la2prd[la] = (int32_t)o->prdIdxs.size();
            o->prdIdxs.push_back(la);
        }
    const int Nprd = (int)o->prdIdxs.size();
    o->JRest = (double*)std::calloc((size_t)Nprd * Ns, sizeof(double));
    if (!o->JRest)
        return fail(LWHIP_ERR_INVALID, "lwhip_hprd_build: out of host memory");

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(LWHIP_ERR_DEVICE, "lwhip_hprd_build: no HIP device visible (this library has no CPU path)");
    const int device = opts ? opts->device : 0;
    if (device < 0 || device >= ndev)
        return fail(LWHIP_ERR_INVALID, "lwhip_hprd_build: bad device ordinal");
    HIP_TRY(hipSetDevice(device));
    hipStream_t stream = opts ? (hipStream_t)opts->stream : nullptr, own = nullptr;
    if (!stream)
    {
        HIP_TRY(stream_acquire(device, &own));
        stream = own;
    }
    // (the device buffers of hprd_build_device are gone, and the stream waited for, before it goes back to the pool)
    int st = hprd_build_device(p, la2prd, lines, lineWave, nRho, stream, *o);
    if (st != LWHIP_OK)
        (void)hipStreamSynchronize(stream);
    if (own)
        stream_release(device, own);
    if (st != LWHIP_OK)
        return st;
    o->rhoPtrs.resize(Nl);
    for (int q = 0; q < Nl; ++q)
        o->rhoPtrs[q] = o->rho + lines[q].cellOff;
    lwhip_hprd& h = o->h;
    h.NprdLambda = Nprd;
    h.Nlines = Nl;
    h.prdIdxs = o->prdIdxs.data();
    h.hPrdIdxs = o->hPrdIdxs.data();
    h.JRest = o->JRest;
    h.jCoeffOff = o->off;
    h.jCoeffs = o->jc;
    h.lineAtom = o->lineAtom.data();
    h.lineTrans = o->lineTrans.data();
    h.rhoCoeffs = o->rhoPtrs.data();
    *out = &o.release()->h;
    return LWHIP_OK;
}

void lwhip_hprd_free(lwhip_hprd* tables)
{
    if (!tables)
        return;
    HprdOwned* o = reinterpret_cast<HprdOwned*>(tables);
    if (o->magic != HPRD_MAGIC)
        return; // (not one of lwhip_hprd_build's: its owner frees it)
    o->magic = 0;
    delete o;
}
