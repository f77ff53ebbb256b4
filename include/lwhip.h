/*
 * lwhip.h -- C ABI of the MI355X (gfx950) implementation of Lightweaver's
 * `formal_sol_gamma_matrices` iteration (1D plane-parallel, unpolarised).
 *
 * This is the drop-in boundary.  Everything above it (the Lightweaver plugin
 * `fs_iteration_fns_provider`, the Python ctypes mirror) talks to the HIP
 * kernels only through the functions declared here: plain pointers and sizes,
 * no C++ types, no torch types.
 *
 * Each entry point names the reference interface it replaces (paths relative
 * to the Lightweaver source tree):
 *
 *   lwhip_formal_sol_gamma_matrices  <- FsIterationFns::fs_iter
 *        (Source/LwFormalInterface.hpp:86,118; trampoline Source/FormalScalar.cpp:678-681;
 *         scalar body Source/SimdFullIterationTemplates.hpp:588-719)
 *   lwhip_formal_sol                 <- FsIterationFns::simple_fs
 *        (Source/LwFormalInterface.hpp:87,119; Source/SimdFullIterationTemplates.hpp:721-781)
 *   lwhip_stat_equil                 <- FsIterationFns::stat_eq
 *        (Source/LwFormalInterface.hpp:91,122; Source/UpdatePopulations.cpp:7-47; Source/LuSolve.cpp:8-132)
 *   lwhip_compute_profiles           <- Transition::compute_phi / compute_wphi
 *        (Source/FormalScalar.cpp:28-68,106-134)
 *   lwhip_redistribute_prd           <- FsIterationFns::redistribute_prd
 *        (Source/LwFormalInterface.hpp:90,121; Source/PrdTemplates.hpp:175-351; Source/Prd.cpp:9-30,51-124,180-263,468-645)
 *   lwhip_create / lwhip_destroy     <- FsIterationFns::alloc_global_scratch / free_global_scratch
 *        (Source/LwFormalInterface.hpp:106-107,131-132; called from Source/ThreadStorage.cpp:480-493,538-566)
 *   lwhip_upload / lwhip_download    <- (none: the reference shares host memory; these move the
 *        borrowed numpy buffers of Source/LwMiddleLayer.pyx to/from HBM)
 *
 * The problem descriptor is a flat restatement of what `Context&` reaches
 * (Source/LwContext.hpp:20-46): Atmosphere (Source/LwAtmosphere.hpp:179-221), Spectrum and
 * Background (Source/LwMisc.hpp:85-110), Atom (Source/LwAtom.hpp:41-80) and Transition
 * (Source/LwTransition.hpp:21-69).  All arrays are C-contiguous fp64, depth `k` fastest,
 * exactly as the reference lays them out.
 *
 * All host pointers in the descriptor are BORROWED: the library reads them in
 * lwhip_create/lwhip_upload and writes them in lwhip_download, never otherwise.
 */
#ifndef LWHIP_H
#define LWHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LWHIP_ABI_VERSION 4

/* ---- enums (values mirror the reference where one exists) ---------------- */

/* TransitionType, Source/LwTransition.hpp:10-14 */
enum { LWHIP_LINE = 0, LWHIP_CONTINUUM = 1 };

/* RadiationBc, Source/LwAtmosphere.hpp:6-13 */
enum {
    LWHIP_BC_UNINITIALISED = 0,
    LWHIP_BC_ZERO = 1,
    LWHIP_BC_THERMALISED = 2,
    LWHIP_BC_PERIODIC = 3,
    LWHIP_BC_CALLABLE = 4
};

/* 1D formal solvers registered in Source/FormalInterface.cpp:30-32 */
enum {
    LWHIP_FS_LINEAR_1D = 0,  /* "piecewise_linear_1d"  */
    LWHIP_FS_BESSER_1D = 1,  /* "piecewise_besser_1d"  */
    LWHIP_FS_BEZIER3_1D = 2  /* "piecewise_bezier3_1d" (reference default, lightweaver/config.py:12) */
};

/* status codes */
enum {
    LWHIP_OK = 0,
    LWHIP_ERR_INVALID = 1,      /* bad descriptor / argument                       */
    LWHIP_ERR_UNSUPPORTED = 2,  /* valid in the reference, not built here (stated)   */
    LWHIP_ERR_DEVICE = 3,       /* HIP runtime failure or no gfx950 device          */
    LWHIP_ERR_SINGULAR = 4,     /* "Singular Matrix" of Source/LuSolve.cpp:22-23       */
    LWHIP_ERR_BUSY = 5          /* lwhip_destroy of a context whose tables are still borrowed (lwhip_create_like) */
};

/* array groups for lwhip_upload / lwhip_download (bit mask) */
enum {
    LWHIP_ATMOS      = 1 << 0,  /* height, temperature, muz, wmu, vlosMu, wavelength   (up)     */
    LWHIP_BACKGROUND = 1 << 1,  /* background chi, eta, sca                             (up)     */
    LWHIP_PROFILES   = 1 << 2,  /* phi, wphi of every line                              (up/down)*/
    LWHIP_POPS       = 1 << 3,  /* n of every atom                                      (up/down)*/
    LWHIP_NSTAR      = 1 << 4,  /* nStar, nTotal, vBroad of every atom, aDamp of lines   (up)     */
    LWHIP_J          = 1 << 5,  /* spect.J                                              (up/down)*/
    LWHIP_GAMMA      = 1 << 6,  /* Gamma of every active atom (pre-fill in, result out) (up/down)*/
    LWHIP_BC         = 1 << 7,  /* CALLABLE boundary data                               (up)     */
    LWHIP_RHOPRD     = 1 << 8,  /* rhoPrd of PRD lines                                  (up)     */
    LWHIP_I          = 1 << 9,  /* spect.I                                              (down)   */
    LWHIP_RATES      = 1 << 10, /* Rij, Rji of every transition                         (down)   */
    LWHIP_DEPTHDATA  = 1 << 11, /* depthData chi, eta, I (only when requested at create)(down)   */
    LWHIP_COLLISIONS = 1 << 12, /* C of every active atom                               (up)     */
    LWHIP_STOKES     = 1 << 13, /* lwhip_stokes: B, projections, J20 (up); phiQ..psiV of every polarised line (up/down);
                                 * Quv, J20 (down).  Not part of LWHIP_ALL_*; ignored without lwhip_set_stokes           */
    LWHIP_ALL_INPUTS = (1 << 0) | (1 << 1) | (1 << 2) | (1 << 3) | (1 << 4) | (1 << 5) | (1 << 6) |
                       (1 << 7) | (1 << 8) | (1 << 12),
    LWHIP_ALL_OUTPUTS = (1 << 5) | (1 << 6) | (1 << 9) | (1 << 10)
};

/* ---- descriptor ----------------------------------------------------------- */

/* One radiative transition; mirrors Transition (Source/LwTransition.hpp:21-69). */
typedef struct lwhip_transition {
    int32_t type;          /* LWHIP_LINE | LWHIP_CONTINUUM                                         */
    int32_t i, j;          /* lower, upper level                                                   */
    int32_t Nblue, Nred;   /* active for Nblue <= la < Nred of the global grid (is_active, :88-91)   */
    int32_t prd;           /* non-zero: rhoPrd is valid and multiplies gij (LwAtom.hpp:121-123)    */
    double Aji, Bji, Bij;  /* Einstein coefficients (lines)                                        */
    double lambda0;        /* [nm]                                                                 */
    double dopplerWidth;   /* c/lambda0 for lines, 1.0 for continua (LwMiddleLayer.pyx:1799,1815)  */
    const double* wavelength; /* [Nred-Nblue] = global wavelength[Nblue:Nred]                      */
    const double* alpha;   /* [Nred-Nblue] cross-section, continua only                            */
    double* phi;           /* [Nred-Nblue, Nrays, 2, Nspace] lines only; dir 0 = down, 1 = toObs   */
    double* wphi;          /* [Nspace] lines only                                                  */
    const double* aDamp;   /* [Nspace] lines only; needed by lwhip_compute_profiles                */
    double* rhoPrd;        /* [Nred-Nblue, Nspace] or NULL                                         */
    double* Rij;           /* [Nspace] out                                                         */
    double* Rji;           /* [Nspace] out                                                         */
    const double* Qelast;  /* [Nspace] elastic collision rate, PRD lines only (Prd.cpp:18)          */
} lwhip_transition;

/* One atom; mirrors Atom (Source/LwAtom.hpp:41-80). */
typedef struct lwhip_atom {
    int32_t Nlevel;
    int32_t Ntrans;
    int32_t detailed;      /* non-zero: member of ctx.detailedAtoms (rates only, no Gamma)         */
    int32_t _pad;
    double* n;             /* [Nlevel, Nspace] in; out of lwhip_stat_equil                         */
    const double* nStar;   /* [Nlevel, Nspace]                                                     */
    const double* nTotal;  /* [Nspace]                                                             */
    const double* vBroad;  /* [Nspace]                                                             */
    double* Gamma;         /* [Nlevel, Nlevel, Nspace] index (to, from, k); NULL if detailed       */
    const double* C;       /* [Nlevel, Nlevel, Nspace] collisional rates; may be NULL              */
    lwhip_transition* trans; /* [Ntrans]                                                           */
} lwhip_atom;

/* One z boundary; mirrors AtmosphericBoundaryCondition (Source/LwAtmosphere.hpp:17-43). */
typedef struct lwhip_boundary {
    int32_t type;          /* LWHIP_BC_*                                                           */
    int32_t Nmu;           /* second extent of bcData                                              */
    const int32_t* idxs;   /* [Nrays, 2] -> row of bcData, or -1 (CALLABLE only)                   */
    const double* bcData;  /* [Nlambda, Nmu] (third reference extent is 1 in 1D; [Nlambda, Nmu, Nz] for the x
                            * boundaries of a 2D grid) (CALLABLE only)                              */
} lwhip_boundary;

struct lwhip_grid2d; /* 2D geometry, defined below */

typedef struct lwhip_problem {
    int32_t abiVersion;    /* LWHIP_ABI_VERSION                                                    */
    int32_t Nspace;        /* depth points                                                         */
    int32_t Nrays;         /* mu quadrature points                                                 */
    int32_t Nlambda;       /* global wavelength grid                                               */
    int32_t Natom;         /* active atoms first, then detailed atoms                              */
    int32_t formalSolver;  /* LWHIP_FS_*                                                           */
    int32_t storeDepthData;/* non-zero: fill depthChi/depthEta/depthI (DepthData.fill)             */
    int32_t _pad;
    const double* height;      /* [Nspace] m, decreasing index 0 = top                              */
    const double* temperature; /* [Nspace] K                                                        */
    const double* vlosMu;      /* [Nrays, Nspace]; needed by lwhip_compute_profiles only            */
    const double* muz;         /* [Nrays]                                                           */
    const double* wmu;         /* [Nrays]                                                           */
    const double* wavelength;  /* [Nlambda] nm                                                      */
    lwhip_boundary zLowerBc;   /* bottom of the atmosphere (k = Nspace-1), feeds up-going rays      */
    lwhip_boundary zUpperBc;   /* top (k = 0), feeds down-going rays                                */
    const double* bgChi;       /* [Nlambda, Nspace]                                                 */
    const double* bgEta;       /* [Nlambda, Nspace]                                                 */
    const double* bgSca;       /* [Nlambda, Nspace]                                                 */
    double* J;                 /* [Nlambda, Nspace] in (J-dagger) / out                             */
    double* I;                 /* [Nlambda, Nrays] out, emergent intensity at k = 0                 */
    double* depthChi;          /* [Nlambda, Nrays, 2, Nspace] or NULL                               */
    double* depthEta;          /* [Nlambda, Nrays, 2, Nspace] or NULL                               */
    double* depthI;            /* [Nlambda, Nrays, 2, Nspace] or NULL                               */
    lwhip_atom* atoms;         /* [Natom]                                                           */
    /* 2D (tier 2): non-NULL selects the x-periodic 2D geometry.  Then Nspace = Nz * Nx (index k * Nx + j),
     * the formal solver is piecewise_besser_2d with interp_linear_2d whatever formalSolver says, `height` is
     * unused, the z boundaries come from the grid, and I is [Nlambda, Nrays, Nx] (the top row of every
     * column, Spectrum::I with Noutgoing = Nx).  Not supported on the device yet (LWHIP_ERR_UNSUPPORTED). */
    const struct lwhip_grid2d* grid2d;
} lwhip_problem;

/* Hybrid PRD (Leenaarts et al. 2012): what configure_hprd_coeffs (Source/Prd.cpp:697-946) leaves in Spectrum
 * (prdIdxs, hPrdIdxs, JRest, JCoeffs; Source/LwMisc.hpp:92-104) and in every PRD line (hPrdCoeffs,
 * Source/LwTransition.hpp:65), flattened.  With it a context
 *   - multiplies V_ji of a PRD line by rho interpolated to the ray's rest wavelength,
 *     rho = (1 - frac) rhoPrd(i0, k) + frac rhoPrd(i1, k)   (Transition::uv, Source/LwTransition.hpp:116-127)
 *     instead of by rhoPrd(lt, k) (Source/LwAtom.hpp:118-123),
 *   - scatters every ray's intensity into the rest-frame mean intensity,
 *     JRest(idx, k) += 0.5 wmu frac I(k)   (Source/SimdFullIterationTemplates.hpp:397-408),
 *   - takes J of the scattering integral from JRest (Source/Prd.cpp:384-389, 484-490),
 *   - visits hPrdIdxs in the PRD rates pass (Source/PrdTemplates.hpp:234-248).
 * All arrays are borrowed for the life of the context; JRest is written by lwhip_download(LWHIP_J). */
typedef struct lwhip_rho_coeff {   /* Prd::RhoInterpCoeffs, Source/LwMisc.hpp:50-57 */
    int32_t i0, i1;
    double frac;
} lwhip_rho_coeff;
typedef struct lwhip_j_coeff {     /* Prd::JInterpCoeffs, Source/LwMisc.hpp:58-64 */
    double frac;
    int32_t idx;                   /* row of JRest */
    int32_t _pad;
} lwhip_j_coeff;
typedef struct lwhip_hprd {
    int32_t NprdLambda;            /* spect.prdIdxs.size(): wavelengths where a PRD line is active = rows of JRest  */
    int32_t NhPrd;                 /* spect.hPrdIdxs.size(): wavelengths that scatter into them                     */
    int32_t Nlines;                /* PRD lines that carry hPrdCoeffs                                                */
    int32_t _pad;
    const int32_t* prdIdxs;        /* [NprdLambda] global wavelength indices, increasing                             */
    const int32_t* hPrdIdxs;       /* [NhPrd]                                                                        */
    double* JRest;                 /* [NprdLambda, Nspace] out                                                       */
    const int64_t* jCoeffOff;      /* [NhPrd * Nrays * 2 * Nspace + 1]: where JCoeffs(hPrdLa, mu, toObs, k) starts   */
    const lwhip_j_coeff* jCoeffs;  /* the entries, back to back                                                      */
    const int32_t* lineAtom;       /* [Nlines] index into prob->atoms                                                */
    const int32_t* lineTrans;      /* [Nlines] index into that atom's trans                                          */
    const lwhip_rho_coeff* const* rhoCoeffs; /* [Nlines] -> [Nred - Nblue, Nrays, 2, Nspace]                         */
} lwhip_hprd;

#define LWHIP_OPT_PRD_DETAILED (1 << 16)
/* Gamma and the rates summed in a fixed order (bit-reproducible run to run, as the reference's single-thread path and
 * its fixed-order thread reduction are, Source/ThreadStorage.cpp:343-396): per-workgroup partial slabs added in
 * workgroup order instead of fp64 atomics.  Served by the depth-across-lanes sweep with one wavefront per workgroup
 * (contexts it does not cover -- other solvers than Bezier3, column batches -- ignore the flag); J and I are
 * reproducible either way.  Costs a factor 2-4 in the sweep (one wavefront per workgroup): off by
 * default, also in the plugin (LWHIP_DETERMINISTIC=1 turns it on there and in any context). */
#define LWHIP_OPT_DETERMINISTIC (1 << 17)

typedef struct lwhip_options {
    int32_t device;        /* HIP device ordinal                                                   */
    int32_t laStart;       /* wavelength shard owned by this context: [laStart, laEnd)             */
    int32_t laEnd;         /* 0,0 = whole grid                                                     */
    int32_t flags;         /* bits 0-15: column-batch hint = number of contexts that will share the device
                            * through lwhip_batch_* (0: none; sizes the per-context chunking);
                            * bit 16 (LWHIP_OPT_PRD_DETAILED): the PRD calls include the PRD lines of
                            * detailed-static atoms -- ExtraParams "include_detailed_atoms" of
                            * redistribute_prd_lines (Source/PrdTemplates.hpp:25-29, 190-215), the default of
                            * LwContext.prd_redistribute (Source/LwMiddleLayer.pyx:3678-3680); rest reserved */
    int32_t worldSize;     /* number of wavelength shards of the job (0 or 1 = unsharded)          */
    int32_t worldRank;     /* this shard's ordinal: selects its (dJMax, idx) slot in the buffer    */
    void* stream;          /* hipStream_t to launch on, NULL = the library's own stream            */
    const lwhip_hprd* hprd;/* hybrid PRD tables (configure_hprd_coeffs was called on the Context), or NULL */
} lwhip_options;

typedef struct lwhip_context lwhip_context; /* opaque */

/* Result of one iteration; the members of IterationResult (Source/LwIterationResult.hpp:6-28)
 * that fs_iter fills (Source/SimdFullIterationTemplates.hpp:633-637). */
typedef struct lwhip_iter_result {
    int32_t updatedJ;
    int32_t dJMaxIdx;      /* wavelength index of the first maximum of dJ(la)                      */
    double dJMax;          /* max_la max_k |1 - Jdag/J|                                            */
} lwhip_iter_result;

/* ---- entry points ----------------------------------------------------------- */

/* Text of the last error raised on the calling thread ("" if none). */
const char* lwhip_last_error(void);

/* ---- the caller's J array as a direct output of the sweep (drop-in mode) -------------------------------------------------
 * lwhip_map_host_J(ctx, 1) page-locks the problem's J array ([Nlambda, Nspace], hipHostRegister) and from then on the sweep
 * stores every J it forms into the device's copy AND straight into that array (stores over PCIe, spread over the kernel's
 * duration): `lwhip_download(LWHIP_J)` then moves nothing -- the 6.7 MB copy of J at 10 240 wavelengths was the largest part
 * of a host-authoritative call.  The array holds the new J once the stream has been waited for (every download does).
 * 1D problems on the depth-across-lanes sweep, unsharded; LWHIP_ERR_UNSUPPORTED otherwise or when the registration fails (the
 * caller goes on with copies).  lwhip_map_host_J(ctx, 0) -- and lwhip_destroy -- release the registration; call it before
 * the array is freed or replaced.  Contract served: `spect.J` overwritten for all wavelengths when fs_iter returns
 * (Source/LwMiddleLayer.pyx:3198-3207, Source/SimdFullIterationTemplates.hpp:181-190). */
int lwhip_map_host_J(lwhip_context* ctx, int enable);

/* Exact change detection without reading J back: the 64-bit fingerprint lwhip_host_fingerprint(p, n) would give for the
 * DEVICE's current J if it were copied into an array at address `p` (n = Nla * Nspace doubles of the shard), computed on the
 * device (one pass over J in HBM, a few microseconds) -- so a host-authoritative caller can tell at its next call, from a
 * fingerprint of its own array, whether anybody rewrote `spect.J` in between, and skip the upload of J when nobody did.
 * The fingerprint is defined here: the array in blocks of LWHIP_FP_BLOCK doubles, per block a Fletcher-style pair of running
 * sums over 8 interleaved 64-bit lanes (lwhip_fp_block_sums), folded with lwhip_fp_mix in block order.  Any change of one
 * element changes it. */
int lwhip_fingerprint_J(lwhip_context* ctx, const void* p, uint64_t* out);
/* A copy of the device's J kept on the device / put back (stream-ordered, a few microseconds): with a mapped J array the sweep
 * overwrites the caller's copy of the J an iteration starts from, so a caller that may have to run the iteration a second time
 * on corrected inputs (the plugin's speculative run, lwhip_plugin.cpp fs_iter_hip) takes the starting J back from here. */
int lwhip_j_snapshot(lwhip_context* ctx);
int lwhip_j_restore(lwhip_context* ctx);
uint64_t lwhip_host_fingerprint(const double* p, size_t n);

enum { LWHIP_FP_BLOCK = 32768 };
static inline uint64_t lwhip_fp_mix(uint64_t h, uint64_t bits)
{
    h = (h ^ bits) * 0x9E3779B97F4A7C15ull;
    return h ^ (h >> 29);
}
/* one block's fingerprint from its 16 sums (s1[8], s2[8]), its length and its offset in the array */
static inline uint64_t lwhip_fp_block_fold(const uint64_t* sums, size_t n, uint64_t offset)
{
    uint64_t h = lwhip_fp_mix(1469598103934665603ull ^ offset, (uint64_t)n);
    for (int l = 0; l < 8; ++l)
        h = lwhip_fp_mix(lwhip_fp_mix(h, sums[l]), sums[8 + l]);
    return h;
}
/* the array's fingerprint from its blocks' fingerprints */
static inline uint64_t lwhip_fp_array_fold(const uint64_t* blockHashes, size_t nBlocks, const void* p, size_t n)
{
    uint64_t h = lwhip_fp_mix((uint64_t)(uintptr_t)p, (uint64_t)n);
    for (size_t b = 0; b < nBlocks; ++b)
        h = lwhip_fp_mix(h, blockHashes[b]);
    return h;
}

/* Diagnosis (LWHIP_DEBUG set in the environment): the pinned host blocks of destroyed contexts are kept and filled with a
 * pattern instead of being given back to the runtime; this returns the number of their bytes that no longer hold it (0 = nothing
 * stored into host memory of a context that was gone) and prints the first few to stderr.  Without LWHIP_DEBUG there is no
 * quarantine and the answer is 0.  Also run when the process ends.  No counterpart in the reference. */
long lwhip_debug_check_quarantine(void);

/* Streams the library has created with hipStreamCreate in this process so far.  Contexts' own streams are POOLED per device
 * and never destroyed (a context that dies gives its stream to the next one): the HIP runtime's completion callback may store
 * into a stream's queue object after hipStreamDestroy has freed it (profiles/r06_stray_write.md), i.e. into whatever host
 * allocation reuses that block.  Making and closing contexts one after the other leaves this count at the number that were
 * alive at the same time (tests/test_abi.py).  No counterpart in the reference. */
long lwhip_debug_streams_created(void);

/* ABI version the library was built with. */
int lwhip_abi_version(void);

/* Number of visible gfx950 devices (0 if none / no driver). Never fails. */
int lwhip_device_count(void);

/* Allocate device state for `prob`, build the per-wavelength activity tables and upload
 * LWHIP_ALL_INPUTS.  Replaces alloc_global_scratch.  `opts` may be NULL. */
int lwhip_create(const lwhip_problem* prob, const lwhip_options* opts, lwhip_context** out);

/* The same for a problem of the SAME STRUCTURE as the one `like` was made for -- sizes, solver, wavelength shard and grid, and
 * of every transition its levels, wavelength range, coefficients, own grid and cross-sections; populations, atmosphere,
 * profiles, boundary data are free to differ: the columns of a 1.5D batch, lwhip_batch_create.  The new context borrows
 * `like`'s structure tables (per-wavelength activity tables, tile / workgroup / ray records: a few MB and half of the
 * creation time per context) instead of building device copies of its own.  The structures are compared by a fingerprint:
 * LWHIP_ERR_INVALID if they differ.  `like` cannot be destroyed before its borrowers (lwhip_destroy fails with
 * LWHIP_ERR_BUSY and leaves it intact).  No counterpart in the reference: every Context owns its tables
 * (update_deps, Source/LwMiddleLayer.pyx:3244-3288). */
int lwhip_create_like(const lwhip_problem* prob, const lwhip_options* opts, lwhip_context* like, lwhip_context** out);

/* Free everything lwhip_create allocated.  Replaces free_global_scratch. */
int lwhip_destroy(lwhip_context* ctx);

/* The hybrid PRD tables of a problem, built on the device: configure_hprd_coeffs (Source/Prd.cpp:697-946; what
 * LwContext(hprd=True) calls at construction and again whenever the velocity field changes, Source/LwMiddleLayer.pyx:3686-3720).
 * *out receives a library-owned lwhip_hprd -- exactly what lwhip_create takes through lwhip_options.hprd, the reference's
 * tables bit for bit (the build needs only correctly rounded fp64 multiply, divide, add and compare) -- whose JRest is its own
 * zeroed [NprdLambda, Nspace] array.  Contexts borrow the tables: free them with lwhip_hprd_free after those contexts are
 * destroyed (NULL is a no-op; tables from anywhere else are left alone).
 * The lines: every LWHIP_LINE with prd and rhoPrd, active atoms first, with includeDetailed followed by those of the detailed
 * atoms (:712-735).  A problem without such a line: LWHIP_OK and *out = NULL (the reference returns early and stays plain PRD).
 * Of `opts` only device and stream are read (NULL: device 0, a stream of the library's).  Refused before the device is
 * touched, *out = NULL: a null prob or out, an ABI version mismatch, a problem without vlosMu or wavelength, a PRD line with
 * fewer than 2 wavelengths (LWHIP_ERR_INVALID); a 2D problem (LWHIP_ERR_UNSUPPORTED).  Without a HIP device: LWHIP_ERR_DEVICE,
 * there is no CPU path.  On the stream: one upload of the inputs (both grids, vlosMu, a few KB), the launches, and three waits
 * -- for the per-wavelength flags the layout depends on, for the 8-byte total that sizes jCoeffs, for the tables. */
int lwhip_hprd_build(const lwhip_problem* prob, const lwhip_options* opts, int includeDetailed, lwhip_hprd** out);
void lwhip_hprd_free(lwhip_hprd* tables);

/* Copy the host arrays named by `mask` (LWHIP_* bits) from the descriptor given at create
 * into HBM / back out of it.  Synchronous with respect to the host buffers. */
int lwhip_upload(lwhip_context* ctx, uint32_t mask);
int lwhip_download(lwhip_context* ctx, uint32_t mask);

/* Gamma <- crsw * C on the device: the pre-fill LwContext.formal_sol_gamma_matrices performs on
 * the host before calling the core (Source/LwMiddleLayer.pyx:3198-3203). */
int lwhip_gamma_prefill_from_C(lwhip_context* ctx, double crsw);

/* lwhip_gamma_prefill_from_C(crsw) followed by lwhip_formal_sol_gamma_matrices in one call: the device-resident iteration of
 * LwContext.formal_sol_gamma_matrices (Source/LwMiddleLayer.pyx:3152-3210: Gamma <- crsw C, then the scheme's fs_iter). */
int lwhip_iterate_from_C(lwhip_context* ctx, int lambdaIterate, double crsw, lwhip_iter_result* res);

/* One formal_sol_gamma_matrices iteration over the context's wavelength shard:
 * J, I overwritten, Rij/Rji fresh integrals, Gamma += radiative terms, diagonal finalised.
 * Pre-condition (as in the reference): Gamma holds the collisional pre-fill.
 * `lambdaIterate` != 0 sets PsiStar = 0 (FsMode::PureLambdaIteration). */
int lwhip_formal_sol_gamma_matrices(lwhip_context* ctx, int lambdaIterate, lwhip_iter_result* res);

/* The same iteration split around the cross-GPU reduction (wavelength-sharded runs):
 *   lwhip_fs_partial   launches the sweep; leaves this shard's Gamma/R partial sums in the first
 *                      `nSum` doubles of the reduce buffer and its (dJMax, idx) in slot `worldRank`
 *                      of the `nGather` = 2*worldSize trailing doubles (all other slots zero);
 *   (caller all-reduces -- SUM -- the whole buffer of nSum + nGather doubles: one collective)
 *   lwhip_fs_finalise  adds the reduced sums into Gamma (which keeps its pre-fill, cf.
 *                      Source/ThreadStorage.cpp:155-156), finalises the diagonal, writes Rij/Rji. */
int lwhip_fs_partial(lwhip_context* ctx, int lambdaIterate);
int lwhip_fs_finalise(lwhip_context* ctx, lwhip_iter_result* res);
/* Device pointer and layout of the reduce buffer: [0,nSum) partial sums, [nSum,nSum+nGather) the
 * per-rank (dJMax, idx) slots. */
int lwhip_reduce_buffer(lwhip_context* ctx, void** devPtr, size_t* nSum, size_t* nGather);

/* The same exchange WITHOUT a collective call, for the ranks of one node (one process per GPU, or several contexts of one
 * process): every rank owns a window in device memory; lwhip_fs_partial then stores the rank's partial sums into its slot of
 * EVERY rank's window (peer-mapped stores: xGMI between GPUs) and raises its flag there, and lwhip_fs_finalise's launch waits for
 * the worldSize flags of its own window and adds the slots IN RANK ORDER -- so sharded Gamma / rates are the same bits on every
 * rank and from run to run (with the fixed-order mode for the sums inside a shard), which the summation tree of a library
 * all-reduce does not promise.  Replaces AtomStorageFactory::accumulate_Gamma / TransitionStorageFactory::accumulate_rates
 * across threads (Source/ThreadStorage.cpp:150-166, 334-396; called from Source/SimdFullIterationTemplates.hpp:675-703).
 *   lwhip_peer_window           allocates (once) and returns this rank's window;
 *   lwhip_peer_export           the window's inter-process handle (hipIpcMemHandle_t as 64 opaque bytes) -- the caller ships it
 *                               to the other ranks (e.g. torch.distributed.all_gather_object) ...
 *   lwhip_peer_attach           ... and hands in all worldSize handles, own rank's entry ignored: from now on fs_partial /
 *                               fs_finalise exchange through the windows and the caller must NOT all-reduce the reduce buffer;
 *   lwhip_peer_attach_pointers  the same for windows the process can address directly (contexts of ONE process: pointers
 *                               from lwhip_peer_window, peer access enabled by the caller where they live on other devices);
 *   lwhip_peer_detach           waits for the stream and goes back to the all-reduce contract.
 * All ranks must make the same sequence of fs_partial / fs_finalise calls while attached.  A rank whose peers never publish
 * (a dead process) does not hang the device: the launch gives up after ~2 s and lwhip_fs_finalise reports LWHIP_ERR_DEVICE.
 * The PRD calls (lwhip_prd_pack / _partial / _finalise) keep the all-reduce contract. */
int lwhip_peer_window(lwhip_context* ctx, void** devPtr, size_t* bytes);
int lwhip_peer_export(lwhip_context* ctx, void* handle64);
int lwhip_peer_attach(lwhip_context* ctx, const void* handles /* worldSize x 64 bytes */);
int lwhip_peer_attach_pointers(lwhip_context* ctx, void* const* windows /* worldSize device pointers */);
int lwhip_peer_detach(lwhip_context* ctx);
/* One exchange of a known per-rank pattern instead of the partial sums -- called by ALL attached ranks together, before the
 * exchange is relied on: *result = 0 every rank's slot arrived intact within timeoutMs, 1 a rank's flag never came, 2 a slot
 * holds something else (stores of a peer not visible to this device's kernels).  What a caller does on a non-zero result is
 * detach everywhere and fall back to the all-reduce (lightweaver_amd.distributed.ShardedIteration does).  The windows are
 * uncached / fine-grained device memory where the runtime offers it, so that a peer's stores are seen by a running kernel. */
int lwhip_peer_selftest(lwhip_context* ctx, int timeoutMs, int32_t* result);

/* formal_sol: chi/S/solve/I only, optionally up-going rays only (FsMode::FsOnly|UpOnly).  J, Gamma, the rates and the depth
 * data (storeDepthData) are left as they are, in 1D and in 2D: only the iteration stores depth data. */
int lwhip_formal_sol(lwhip_context* ctx, int upOnly);

/* Statistical equilibrium for atom `atom` (index into prob->atoms; -1 = every active atom):
 * per depth, eliminate the row of the largest population, solve by Crout LU with implicit
 * scaling, partial pivoting and one refinement pass; n overwritten on the device.
 * Returns LWHIP_ERR_SINGULAR where the reference throws "Singular Matrix". */
int lwhip_stat_equil(lwhip_context* ctx, int atom);
/* The same without waiting: the solve is queued on the context's stream and a singular matrix is
 * remembered; lwhip_check_status waits for the stream and returns (and clears) that condition.
 * For batches of contexts whose solves should overlap instead of serialising on a host wait each. */
int lwhip_stat_equil_async(lwhip_context* ctx, int atom);
/* lwhip_stat_equil that also reports, per active atom (arrays indexed by position among the active
 * atoms; entries of atoms not solved are left alone), the maximum relative population change
 * max |(n_new - n_old) / n_new| and the flattened [level, depth] index of its first occurrence: what
 * LwContext.stat_equil returns as dPops / dPopsMaxIdx (Ng::max_change, Source/Ng.hpp:138-156, with the
 * default Ng(0,0,0), i.e. no acceleration). */
int lwhip_stat_equil_report(lwhip_context* ctx, int atom, double* dPops, int32_t* dPopsMaxIdx);
int lwhip_check_status(lwhip_context* ctx);

/* PRD sub-iterations (redistribute_prd_lines): for every PRD line of an active atom, the
 * total depopulation + elastic rate, the angle-averaged scattering integral with Gouttebroze's
 * GII on a 0.15-Doppler-width fine grid (rho <- 1 + gamma (int J gII / int gII - Jbar)), then a
 * formal solution restricted to the PRD wavelengths that updates J and the PRD lines' Rij/Rji;
 * at most maxIter times, until max |d rho / rho| < tol.  rhoPrd, J, Rij/Rji stay on the device.
 * `dRho`/`dRhoMaxIdx` receive one entry per (sub-iteration, PRD line), `dJPrdMax`/`dJPrdMaxIdx`
 * one per sub-iteration; capacities maxIter * Nprd and maxIter (any may be NULL).
 * On a wavelength shard use the split form below (the scattering integral needs J over each PRD
 * line's whole grid, which one all-reduce provides). */
typedef struct lwhip_prd_result {
    int32_t NprdSubIter;
    int32_t Nprd;          /* number of PRD lines */
    double* dRho;
    int32_t* dRhoMaxIdx;
    double* dJPrdMax;
    int32_t* dJPrdMaxIdx;
} lwhip_prd_result;
int lwhip_redistribute_prd(lwhip_context* ctx, int maxIter, double tol, lwhip_prd_result* res);

/* One PRD sub-iteration across wavelength shards ("all-gather J rows of PRD lambda
 * before prd_scatter"), split around its two collectives:
 *   lwhip_prd_pack      this shard's J rows of every PRD line into the gather buffer (zero elsewhere);
 *                       devPtr/count describe it: all-reduce(SUM) it over the shards;
 *   lwhip_prd_partial   rho for this shard's emission wavelengths, max |d rho / rho| per line into this
 *                       shard's slots of the reduce tail, then the PRD rates pass + slab reduce;
 *                       all-reduce(SUM) the buffer of lwhip_reduce_buffer (nSum + nGather doubles);
 *   lwhip_prd_finalise  Rij/Rji of the PRD lines out; per-line (dRho, idx) [Nprd] and (dJMax, idx).
 * lwhip_redistribute_prd is this loop on one device. */
int lwhip_prd_pack(lwhip_context* ctx, void** devPtr, size_t* count);
int lwhip_prd_partial(lwhip_context* ctx);
int lwhip_prd_finalise(lwhip_context* ctx, double* dRho, int32_t* dRhoMaxIdx, double* dJMax, int32_t* dJMaxIdx);

/* Ng acceleration of the populations on the device (struct Ng, Source/Ng.hpp:16-156; driven by
 * LwContext.stat_equil -> rel_diff_ng_accelerate, Source/LwMiddleLayer.pyx:3318-3346).
 * lwhip_ng_configure(Norder, Nperiod, Ndelay): one history per active atom, seeded with the current
 *   populations (the reference builds its Ng objects when the Context is constructed); Norder = 0 keeps
 *   only what max_change needs.
 * lwhip_ng_accelerate: call after each population update: records the new populations, every Nperiod
 *   calls from the Ndelay-th on replaces them by the Ng extrapolation, and reports per active atom whether
 *   it accelerated, the max relative change between the last two recorded solutions and its flattened
 *   [level, depth] index.
 * lwhip_ng_state (reads only): lwhip_batch_ng_state for this one context -- opts[3] = Norder, Nperiod, Ndelay in effect
 *   (Ndelay after the max rule), *count the Ng call count as the device holds it (1 after lwhip_ng_configure),
 *   *lastAccelerated whether the last step extrapolated.  Each may be NULL; not configured: all zero.
 * The history and the call count live on the device; a context is served as a column batch of one column (below). */
int lwhip_ng_configure(lwhip_context* ctx, int Norder, int Nperiod, int Ndelay);
int lwhip_ng_accelerate(lwhip_context* ctx, int32_t* accelerated, double* dPops, int32_t* dPopsMaxIdx);
int lwhip_ng_state(lwhip_context* ctx, int32_t opts[3], int32_t* count, int32_t* lastAccelerated);

/* time_dependent_update (FsIterationFns::time_dep_update, Source/LwFormalInterface.hpp:92,123;
 * time_dependent_update_impl, Source/UpdatePopulations.cpp:120-151): for atom `atom`, per depth
 * point solve (1 - dt Gamma_k) n_k = nOld_k with the solver of lwhip_stat_equil; n overwritten on
 * the device.  nOld: host [Nlevel, Nspace]. */
int lwhip_time_dep_update(lwhip_context* ctx, int atom, const double* nOld, double dt);

/* nr_post_update (FsIterationFns::nr_post_update, Source/LwFormalInterface.hpp:94,124;
 * nr_post_update_impl + F / Ftd, Source/UpdatePopulations.cpp:230-394): one Newton-Raphson step
 * of the coupled statistical-equilibrium (or backward-Euler, when nPrev is given) + charge-
 * conservation system of the listed atoms, per depth point: (sum Nlevel + 1) unknowns, the last
 * one the electron density.  n of the listed atoms is updated on the device, `ne` on the host.
 * Uses the device copies of Gamma and C (collisional rates). */
typedef struct lwhip_nr_args {
    int32_t Natoms;
    int32_t _pad;
    const int32_t* atoms;          /* [Natoms] indices into prob->atoms (active atoms), in equation order */
    const double* const* stages;   /* [Natoms] -> [Nlevel]: ionisation stage of each level (Atom::stages) */
    const double* const* dC;       /* [Natoms] -> [Nlevel, Nlevel, Nspace]: dC/dne, or NULL: no collisional term */
    const double* const* nPrev;    /* [Natoms] -> [Nlevel, Nspace]: previous time step, or NULL: not time dependent */
    const double* backgroundNe;    /* [Nspace] */
    double* ne;                    /* [Nspace] in: atmos.ne; out: ne + delta */
    double dt;                     /* time step (time-dependent form only) */
    double crsw;                   /* collisional-radiative switching value the Gamma pre-fill used */
} lwhip_nr_args;
int lwhip_nr_post_update(lwhip_context* ctx, const lwhip_nr_args* args);

/* spaceStart / spaceEnd of FsIterationFns::stat_eq, time_dep_update and nr_post_update
 * (Source/LwFormalInterface.hpp:90-100; the loops `for k in [spaceStart, spaceEnd)` of
 * Source/UpdatePopulations.cpp:22, :135, :316): the depth range the following lwhip_stat_equil* /
 * lwhip_time_dep_update / lwhip_nr_post_update calls of this context solve; points outside keep their
 * populations (and ne).  (-1, -1) = the whole atmosphere, the state of a new context.  Column batches
 * (lwhip_batch_stat_equil) always solve every point. */
int lwhip_set_depth_range(lwhip_context* ctx, int spaceStart, int spaceEnd);

/* Which wavelength index lwhip_formal_sol_gamma_matrices reports next to dJMax (lwhip_iter_result::dJMaxIdx):
 *   0 (default)  the first wavelength that attains dJMax -- what the reference's threaded schemes return
 *                (the per-thread maxima are merged with max_idx, Source/SimdFullIterationTemplates.hpp:700-715);
 *   1            the bookkeeping of the reference's single-thread branch, bit for bit: its loop calls
 *                `dJMax = max_idx(dJ, dJMax, maxIdx, la)` (Source/SimdFullIterationTemplates.hpp:627 with
 *                Source/Constants.hpp:114-125), which records `la` whenever the wavelength's dJ is BELOW the running
 *                maximum -- i.e. the last wavelength whose dJ is smaller than the largest one before it (0 if there is
 *                none).  The plugin selects it when the Context runs with Nthreads == 1, so a drop-in run reports the
 *                index the scalar scheme reports.  Unsharded 1D contexts; others keep mode 0. */
int lwhip_set_djmax_index_mode(lwhip_context* ctx, int mode);

/* ---- 2D short characteristics (tier 2): the formal solver primitive -------------------
 * piecewise_besser_2d with interp_linear_2d (Source/FormalScalar2d.cpp:740-1184, 209-255) on an x-periodic
 * Nz x Nx grid, given the intersection table the core builds (build_intersection_list, :1188-1327;
 * Atmosphere::intersections, Source/LwAtmosphere.hpp:145-173), flattened as below.  Not yet wired into
 * lwhip_formal_sol_gamma_matrices: this entry point solves chi, S -> I, Psi* for a batch of (ray,
 * direction) pairs. */
#define LWHIP_AXIS_NONE 0
#define LWHIP_AXIS_X 1
#define LWHIP_AXIS_Z 2
typedef struct lwhip_intersection {   /* IntersectionResult, Source/LwAtmosphere.hpp:93-140 */
    int32_t axis;                     /* InterpolationAxis (LWHIP_AXIS_*): 0 none (on a grid point), 1 interpolate along x, 2 along z */
    int32_t _pad;
    double fracZ, fracX;              /* fractional indices of the hit */
    double distance;                  /* path length to it */
} lwhip_intersection;

typedef struct lwhip_grid2d {
    int32_t Nx, Nz, Nrays, periodic;  /* 1: PERIODIC x boundaries; 0: CALLABLE ones (xLowerBc / xUpperBc below)    */
    int32_t zLowerBc, zUpperBc;       /* LWHIP_BC_ZERO / LWHIP_BC_THERMALISED / LWHIP_BC_CALLABLE (then lwhip_problem's
                                       * zLowerBc / zUpperBc carry idxs and bcData [Nlambda, Nmu, Nx])            */
    int32_t NlongChar, _pad;
    const double* x;                  /* [Nx] */
    const double* z;                  /* [Nz] */
    const double* mux;                /* [Nrays] */
    const double* muz;                /* [Nrays] */
    const double* temperature;        /* [Nz, Nx] (thermalised boundaries) */
    const lwhip_intersection* uw;     /* [Nrays, 2, Nz, Nx] upwind hit of every point */
    const lwhip_intersection* dw;     /* [Nrays, 2, Nz, Nx] downwind hit */
    const int32_t* longCharIdx;       /* [Nrays, 2, Nz, Nx] index of the point's long characteristic, or -1 */
    const int32_t* substepOff;        /* [NlongChar + 1] offsets into substeps */
    const lwhip_intersection* substeps; /* the sub-steps of every long characteristic, upwind-most first */
    /* periodic == 0 (Source/FormalScalar2d.cpp:806-852): the column a ray enters through is prescribed,
     * I(k, 0) = xLowerBc.bcData(la, idxs(mu, toObs), k) for mux > 0, I(k, Nx-1) from xUpperBc for mux < 0.
     * Both CALLABLE, idxs [Nrays, 2], bcData [Nlambda, Nmu, Nz]; no long characteristics.  NULL when periodic. */
    const struct lwhip_boundary* xLowerBc;
    const struct lwhip_boundary* xUpperBc;
} lwhip_grid2d;

/* nSolve problems: problem p is ray rays[p] (= 2 * mu + toObs), opacity chi + p * Nz * Nx, source S + ...;
 * writes I and PsiStar (= Psi / chi) of the same shape.  All pointers are host pointers. */
int lwhip_formal_solver_2d(int device, const lwhip_grid2d* grid, double wavelength, int nSolve, const int32_t* rays,
                           const double* chi, const double* S, double* I, double* PsiStar);

/* 1.5D column batches (BASELINE configs[3]): n structurally identical contexts -- same model atoms, wavelength grid,
 * solver and device; own atmospheres, profiles, populations -- advance together, one grid slice per column, on the
 * first column's stream (the others are moved onto it),
 * so a batch of short columns fills the device the way one long wavelength grid does.  Columns never exchange
 * radiation (the reference runs them as separate Contexts: README.md:9); results[i] receives column i's dJMax.
 * Hybrid-PRD columns (lwhip_options.hprd, each with tables for its own velocity field): all columns or none
 * (LWHIP_ERR_INVALID for a mix).  Their tile lists follow their velocities, so on the lane sweep they may differ in their
 * workgroup counts: the one sweep launch takes the largest count and every workgroup checks its own column's
 * (lwhip_batch_sweep_shape); each column's JRest is cleared in front of every pass that rebuilds it. */
typedef struct lwhip_batch lwhip_batch;
int lwhip_batch_create(lwhip_context* const* ctxs, int n, lwhip_batch** out);
void lwhip_batch_destroy(lwhip_batch* batch);
int lwhip_batch_formal_sol_gamma_matrices(lwhip_batch* batch, int lambdaIterate, double crsw,
                                          lwhip_iter_result* results /* [n] or NULL: nothing is read back */);
int lwhip_batch_stat_equil(lwhip_batch* batch);
/* lwhip_compute_profiles of every column, all their lines in one launch pair on the batch's stream (a launch pair per
 * line and column leaves the device empty: 7 680 pairs for 512 columns of 15 lines).  Columns whose atmosphere is
 * uploaded later (LWHIP_ATMOS) are brought up to date the same way by the next lwhip_batch_formal_sol_gamma_matrices. */
int lwhip_batch_compute_profiles(lwhip_batch* batch);

/* Column batches to convergence: the population change per column, and an ACTIVE SET of columns.
 *
 * lwhip_batch_stat_equil_report: lwhip_batch_stat_equil of the active columns that also reports, per column and solved
 * (not detailed) atom, max |(new - old) / new| over the populations and the flattened [level, depth] index of its first
 * occurrence (Ng::max_change, Source/Ng.hpp:138-156: what lwhip_stat_equil_report gives for one context).  dPops and
 * dPopsMaxIdx (or NULL) are [n][Natoms], rows indexed by the ORIGINAL column number, Natoms the number of solved atoms
 * (the same for every column of a batch); rows of inactive columns are left untouched.  On the device every column's
 * per-block maxima are combined by one wavefront (batch_conv_kernel) into one record [dJMax, dJMaxIdx, dPops_0, idx_0,
 * ...] per column -- dJMax as the last lwhip_batch_formal_sol_gamma_matrices left it --, so a reported iteration costs one
 * copy of the records and one stream wait.  lwhip_batch_conv_records copies the records of the last report,
 * [n][2 + 2 Natoms] doubles, rows of columns that were inactive then left untouched; *stride (or NULL) receives
 * 2 + 2 Natoms.  A singular matrix in any active column: LWHIP_ERR_SINGULAR, as lwhip_batch_stat_equil.
 *
 * lwhip_batch_set_active: `columns` is a strictly increasing list of nActive column indices; NULL / 0 restores all columns.
 * Afterwards lwhip_batch_formal_sol_gamma_matrices, lwhip_batch_stat_equil and lwhip_batch_stat_equil_report launch only those
 * columns; their results[i] / rows stay indexed by the original column number and entries of inactive columns are untouched.
 * Every other batch entry point (profiles, Stokes, observer rays, sweep_instance) keeps acting on all columns.  An index out
 * of range, a list that is not strictly increasing, nActive < 0 or nActive > 0 with columns == NULL: LWHIP_ERR_INVALID, the
 * active set left as it was.  lwhip_batch_active reads the set back: columns [n] (or NULL) and *nActive.
 * Three invariants:
 *  - a retired (inactive) column's device state -- J, I, n, Gamma, rates, and with Ng (below) its history and call count --
 *    is exactly what its last iteration left: later batch iterations never touch it;
 *  - the launch-wide choices made "only if every column qualifies" (symmetric / angle-independent profiles, the plain sweep
 *    instance) are evaluated over ALL columns of the batch, not the active ones: the code path a column runs, and so its
 *    bits, do not depend on who else is still active -- the Ng step included: a column's store slot, its accelerate
 *    decision and its coefficients come from its own count and history alone;
 *  - with all columns active the launches and copies of the three entry points are what they were before there was an
 *    active set; and with Ng off they are what they were before there was Ng for batches.
 * The time-dependent and charge-conserving updates of a batch (lwhip_batch_time_dep_update, lwhip_batch_nr_post_update, below)
 * follow the active set under the same invariants, and so do the PRD sub-iterations (lwhip_batch_redistribute_prd, below). */
int lwhip_batch_stat_equil_report(lwhip_batch* batch, double* dPops /* [n][Natoms] */, int32_t* dPopsMaxIdx /* [n][Natoms] or NULL */);
int lwhip_batch_conv_records(lwhip_batch* batch, double* records /* [n][2 + 2 Natoms] */, int* stride /* or NULL */);
int lwhip_batch_set_active(lwhip_batch* batch, const int32_t* columns, int nActive);
int lwhip_batch_active(lwhip_batch* batch, int32_t* columns /* [n] or NULL */, int* nActive);

/* PRD sub-iterations for column batches: every ACTIVE column gets what lwhip_redistribute_prd(ctx, maxIter, tol, ...) gives it
 * alone.  It runs its own sub-iterations and stops after the first whose own largest |d rho / rho| over its lines is below tol,
 * whatever the other columns do: its rho, J and I over the PRD wavelengths and the PRD lines' Rij / Rji are what its own last
 * sub-iteration left.  Lane-sweep batches (columns up to 256 depths) run one set of launches per sub-iteration for all active
 * columns -- five in the steady state, whatever the number of columns: scattering integral, PRD rates pass, sums, rates out,
 * record; six for hybrid-PRD columns, whose JRest is cleared between the integral that reads it and the pass that rebuilds it
 * (a column that has stopped keeps the JRest of its own stop) --; the stopping rule is kept on the device, one word per column, and the sub-iterations are queued in groups of four
 * with one copy and one wait per group.  Batches on the ray-column march run lwhip_redistribute_prd column by column.
 * The arrays of `res` are indexed by the ORIGINAL column number: NprdSubIter [n] (required), dRho / dRhoMaxIdx [n][maxIter][Nprd],
 * dJPrdMax / dJPrdMaxIdx [n][maxIter] (each may be NULL).  Entries of inactive columns, and slots beyond a column's NprdSubIter,
 * stay as the caller filled them; the device state of inactive columns is not touched.  lwhip_batch_conv_records keeps the formal
 * solution's dJMax.  Refused before anything is queued: a null batch or result, an active column with a split iteration or
 * sub-iteration pending or whose PRD atoms have no C (LWHIP_ERR_INVALID); columns made with LWHIP_OPT_PRD_DETAILED, and
 * hybrid-PRD columns that borrow one and the same lwhip_hprd -- they share one host JRest, so each column needs tables of
 * its own -- (LWHIP_ERR_UNSUPPORTED).  maxIter <= 0 or no PRD line: LWHIP_OK, NprdSubIter = 0 for the active columns.
 * The gII cache of a PRD line is per column (it depends on the column's aDamp and vBroad): Nspace * 88 * Nlambda(line) * 10 bytes. */
typedef struct lwhip_batch_prd_result {
    int32_t  Nprd;          /* out: PRD lines per column */
    int32_t  _pad;
    int32_t* NprdSubIter;   /* [n]                  sub-iterations each column ran */
    double*  dRho;          /* [n][maxIter][Nprd]   may be NULL */
    int32_t* dRhoMaxIdx;    /* [n][maxIter][Nprd]   may be NULL */
    double*  dJPrdMax;      /* [n][maxIter]         may be NULL */
    int32_t* dJPrdMaxIdx;   /* [n][maxIter]         may be NULL */
} lwhip_batch_prd_result;
int lwhip_batch_redistribute_prd(lwhip_batch* batch, int maxIter, double tol, lwhip_batch_prd_result* res);

/* Population updates for column batches: lwhip_time_dep_update of every solved atom, and lwhip_nr_post_update, of every ACTIVE
 * column in one launch each, at every depth point (a batch does not follow lwhip_set_depth_range), with the per-column change
 * of what was updated: per column and atom max |(new - old) / new| over the populations with new != 0 and the flattened
 * [level, depth] index of its first occurrence, (0, 0) where nothing changed (LwContext.rel_diff_pops: what the reference's
 * time_dep_update / nr_post_update report).  A call stages everything it sends -- the active columns' argument blocks, then
 * their arrays -- in one pinned block; on the batch's stream it is one copy up, the update launch, batch_conv_kernel, one copy
 * back (the records; for the Newton-Raphson step also ne) and one stream wait.  The records also become those
 * lwhip_batch_conv_records returns (dJMax as the last formal solution left it).  Neither call runs the batch's Ng step or
 * changes its counts and histories.  A column's result does not depend on which other columns are active; a retired column's n
 * and the caller's ne array of it are not touched; dPops / dPopsMaxIdx rows are indexed by the ORIGINAL column number, rows of
 * inactive columns untouched.
 *
 * lwhip_batch_time_dep_update: nOld [n] host pointers, one per column (entries of inactive columns are ignored): the solved
 * atoms' [Nlevel, Nspace] blocks back to back in atom order; dt [n]; dPops / dPopsMaxIdx [n][Natoms] or NULL.
 * lwhip_batch_nr_post_update: perColumn [n], the lwhip_nr_args of lwhip_nr_post_update, one per column (entries of inactive
 * columns are ignored); ne of every active column is updated in place on return.  dPops / dPopsMaxIdx [n][Natoms] or NULL,
 * Natoms the number of SOLVED atoms: the entries of the listed atoms are written, those of solved atoms the call does not list
 * are left untouched (their places in the conv records hold 0).
 * A singular system at a depth point leaves that point's n (and ne) as they were and the call returns LWHIP_ERR_SINGULAR with
 * dPops / dPopsMaxIdx untouched; the other points and columns are updated (ne of every active column is still written).
 * Refused before anything is queued, outputs untouched -- LWHIP_ERR_INVALID: a null batch; a null nOld, dt or perColumn; for an
 * active column a null nOld[i], or null atoms, stages, ne or backgroundNe (or a null entry of stages, nPrev, dC); a listed atom
 * that is detailed, out of range or has no C; a column whose Natoms, atom list or presence of dC / nPrev differs from the
 * first active column's (the message names the column).  LWHIP_ERR_UNSUPPORTED: more than 63 coupled levels. */
int lwhip_batch_time_dep_update(lwhip_batch* batch, const double* const* nOld, const double* dt,
                                double* dPops, int32_t* dPopsMaxIdx);
int lwhip_batch_nr_post_update(lwhip_batch* batch, const lwhip_nr_args* perColumn,
                               double* dPops, int32_t* dPopsMaxIdx);

/* Ng acceleration for column batches: every column behaves as a lone context with lwhip_ng_configure would (struct Ng,
 * Source/Ng.hpp:16-156, driven as LwContext.stat_equil drives it), with its own history and its own call count, both on the
 * device; one launch (ng_kernel, one workgroup per active column and solved atom -- the kernel of lwhip_ng_accelerate, for
 * which a lone context is a batch of one) serves all active columns, whatever their schedules.  This is the BATCH's Ng: it is separate from a column's own lwhip_ng_configure / lwhip_ng_accelerate,
 * which keep acting on that context alone and which the batch never reads.
 *
 * lwhip_batch_ng_configure: validated as lwhip_ng_configure (0 <= Norder <= 6, Nperiod >= 1 when Norder > 0; else
 * LWHIP_ERR_INVALID with the previous configuration kept); Ndelay becomes max(Ndelay, Nperiod + 2).  Stores the current
 * populations of ALL columns, active or not, as their first solution (count = 1) in one launch; a repeated call seeds them
 * again.  (0, 0, 0) turns Ng off and releases the history.
 * While configured, lwhip_batch_stat_equil and lwhip_batch_stat_equil_report run the Ng step of the active columns after
 * their solve, in the same stream and before the one wait; the report's dPops / indices (and the conv records, whose layout
 * does not change) are then Ng's max_change, taken after any extrapolation -- what Context.stat_equil reports with Ng.  A
 * reported iteration still costs one copy and one wait.  A column that is inactive for some calls keeps its schedule, as a
 * lone context whose stat_equil was not called.
 * lwhip_batch_ng_accelerate: the Ng step alone on the active columns (the batch form of lwhip_ng_accelerate): one launch, one
 * copy, one wait.  accelerated [n], dPops and dPopsMaxIdx [n][Natoms] may each be NULL; rows of inactive columns are left
 * untouched.  Before lwhip_batch_ng_configure: LWHIP_ERR_INVALID.  A singular Ng system in an active column:
 * LWHIP_ERR_SINGULAR (outputs untouched); that column's populations are recorded without extrapolation, as
 * lwhip_ng_accelerate leaves them, and the other columns are not affected.
 * lwhip_batch_ng_state (reads only): opts[3] = Norder, Nperiod, Ndelay in effect (Ndelay after the max rule; all zero: off),
 * counts [n] every column's Ng call count as the device holds it, lastAccelerated [n] whether the column's last Ng step
 * extrapolated.  Each may be NULL; off: all zero. */
int lwhip_batch_ng_configure(lwhip_batch* batch, int Norder, int Nperiod, int Ndelay);
int lwhip_batch_ng_accelerate(lwhip_batch* batch, int32_t* accelerated /* [n] or NULL */, double* dPops /* [n][Natoms] or NULL */,
                              int32_t* dPopsMaxIdx /* [n][Natoms] or NULL */);
int lwhip_batch_ng_state(lwhip_batch* batch, int32_t opts[3], int32_t* counts /* [n] or NULL */, int32_t* lastAccelerated /* [n] or NULL */);

/* The intersection table of an x-periodic grid: build_intersection_list (Source/FormalScalar2d.cpp:1188-1327) with
 * dw_intersection_2d (:60-105), uw_intersection_2d (:107-152), uw_intersection_2d_frac_x (:166-206).  Host-side
 * geometry, once per atmosphere; reads Nx, Nz, Nrays, periodic, x, z, mux, muz of `grid`.  Call with uw == NULL to
 * learn the sizes (*nLongChar, *nSubsteps), then with uw, dw, longCharIdx [Nrays, 2, Nz, Nx], substepOff
 * [capLongChar + 1] and substeps [capSubsteps].  Bit-identical to the reference's table. */
int lwhip_build_intersections(const lwhip_grid2d* grid, lwhip_intersection* uw, lwhip_intersection* dw,
                              int32_t* longCharIdx, int32_t* substepOff, int32_t capLongChar,
                              lwhip_intersection* substeps, int64_t capSubsteps, int32_t* nLongChar,
                              int64_t* nSubsteps);

/* Voigt profiles phi and weights wphi of every line, on the device. */
int lwhip_compute_profiles(lwhip_context* ctx);

/* ---- full Stokes (Zeeman-polarised lines), 1D plane-parallel only ------------------------------------------------------
 * What the reference keeps in Atmosphere (B, cosGamma, cos2chi, sin2chi: Source/LwAtmosphere.hpp:190-200), in every polarised
 * Transition (phiQ..psiV, Source/LwTransition.hpp:44-51), in ZeemanComponents (Source/LwMisc.hpp:106-111) and in
 * Spectrum::Quv (Source/LwMisc.hpp:94).  The projections are computed by the caller (Atmosphere::update_projections,
 * Source/Atmosphere.cpp:47-82), as vlosMu is.  All host pointers are BORROWED as in lwhip_problem. */
typedef struct lwhip_stokes_line {
    int32_t atom;          /* index into prob->atoms                                                */
    int32_t trans;         /* index into that atom's trans (a LWHIP_LINE)                           */
    int32_t Ncomp;         /* Zeeman components                                                     */
    int32_t _pad;
    const int32_t* alpha;  /* [Ncomp] -1 sigma_b, 0 pi, 1 sigma_r                                   */
    const double* shift;   /* [Ncomp] in Larmor units                                               */
    const double* strength;/* [Ncomp]                                                               */
    double* phiQ;          /* [Nred-Nblue, Nrays, 2, Nspace] each, in (LWHIP_STOKES up) / out        */
    double* phiU;
    double* phiV;
    double* psiQ;
    double* psiU;
    double* psiV;
} lwhip_stokes_line;

typedef struct lwhip_stokes {
    int32_t Nlines;
    int32_t _pad;
    const double* B;        /* [Nspace] field strength [T]                                           */
    const double* cosGamma; /* [Nrays, Nspace]                                                       */
    const double* cos2chi;  /* [Nrays, Nspace]                                                       */
    const double* sin2chi;  /* [Nrays, Nspace]                                                       */
    const lwhip_stokes_line* lines; /* [Nlines]                                                      */
    double* Quv;            /* [3, Nlambda, Nrays] out: emergent Q, U, V at k = 0                    */
    double* J20;            /* [Nlambda, Nspace] in (J20 dagger) / out, or NULL (ExtraParams "J20")   */
} lwhip_stokes;

/* Borrow `stokes` (NULL: forget it) and upload everything it holds (LWHIP_STOKES).  The descriptor and its line list are
 * copied; the arrays they point to are borrowed for the life of the context or until the next call.  No counterpart in the
 * reference (it shares host memory).  1D unsharded contexts only (LWHIP_ERR_UNSUPPORTED otherwise, also with hybrid PRD
 * tables); LWHIP_ERR_INVALID for a line that is not a line or not in the problem. */
int lwhip_set_stokes(lwhip_context* ctx, const lwhip_stokes* stokes);

/* Transition::compute_polarised_profiles (Source/FormalStokes.cpp:9-117) of every polarised line, on the device: phi, wphi
 * and phiQ..psiV from the complex Faddeeva function w(v + ia) = H + iF.  Overwrites phi and wphi of those lines on the
 * device, as the reference does; lwhip_download(LWHIP_PROFILES | LWHIP_STOKES) brings them back. */
int lwhip_compute_polarised_profiles(lwhip_context* ctx);

/* formal_sol_full_stokes (FsIterationFns::full_stokes_fs, Source/LwFormalInterface.hpp:89; formal_sol_full_stokes_impl and
 * stokes_fs_core, Source/FormalStokes.cpp:418-723): per (lambda, mu, direction) the DELO-Bezier3 march of the 4x4 system, or
 * the scalar piecewise_bezier3_1d where no polarised line is active and there is no J20 -- whatever solver the context was
 * built with.  I [Nlambda, Nrays] and Quv hold the emergent values of the up-going rays (the last ones written, also with
 * upOnly = 0).  updateJ: J and J20 re-accumulated, res->dJMax and res->dJMaxIdx with the single-thread bookkeeping of
 * lwhip_set_djmax_index_mode(1) (the reference's loop is serial: max_idx, Source/FormalStokes.cpp:713).
 * Differences from the reference, stated:
 *   - Q, U, V at a wavelength without a polarised line (and without J20) are exact zeros; the reference stores what the last
 *     polarised ray left in its scratch array there (Source/FormalStokes.cpp:610-616).
 * As in the reference, without updateJ the source function's scattering term uses J dagger = 0 (and J20 dagger = 0): JDag is
 * only filled when J is updated (Source/FormalStokes.cpp:429-438).  Gamma and the rates are never touched.  res may be NULL. */
int lwhip_full_stokes_fs(lwhip_context* ctx, int updateJ, int upOnly, lwhip_iter_result* res);

/* Full Stokes of a 1.5D column batch (lwhip_batch_create): what the two calls above do for one context, for every column of
 * the batch in one set of launches on the batch's stream; each column's results are those of the single-context call on it.
 * Every column needs Stokes data (lwhip_set_stokes) with the polarised lines of column 0 -- the same transitions with the same
 * component counts; B, the projections, J20 and the component values may differ.  No device: LWHIP_ERR_DEVICE; a null
 * batch, a column without Stokes data or with other polarised lines: LWHIP_ERR_INVALID, before anything is launched.
 * lwhip_batch_compute_polarised_profiles: Transition::compute_polarised_profiles of the polarised lines of every column,
 * after the plain profiles of the columns whose atmosphere was uploaded since (as lwhip_compute_polarised_profiles). */
int lwhip_batch_compute_polarised_profiles(lwhip_batch* batch);
/* formal_sol_full_stokes of every column.  results: [n] or NULL (dJMax / dJMaxIdx when updateJ, as res of
 * lwhip_full_stokes_fs).  updateJ while a column has a mapped host J: LWHIP_ERR_UNSUPPORTED.  A singular 4 x 4 system:
 * LWHIP_ERR_SINGULAR naming the first singular column, every column's outputs written all the same. */
int lwhip_batch_full_stokes_fs(lwhip_batch* batch, int updateJ, int upOnly, lwhip_iter_result* results);

/* ---- emergent spectra along observer rays (1D) --------------------------------------------------------------------------
 * LwContext.compute_rays(mus, upOnly=True) (Source/LwMiddleLayer.pyx:3898-4002) from the state resident on the device: for
 * every wavelength of [laStart, laEnd) and every direction cosine muz[m] the up-going ray is traced with piecewise_bezier3_1d
 * through chi and S built as lwhip_formal_sol builds them (lines and continua of the active and detailed atoms from the
 * resident n, background chi / eta / sca, S = (eta + sca J) / chi with the resident J, gij rhoPrd for PRD lines), except that
 * each line's profile is evaluated inside the kernel for the new direction: phi = H(aDamp, v) / (sqrt(pi) vBroad),
 * v = ((lambda - lambda0) c / lambda0 + mu v_z) / vBroad.  The directions need not be quadrature nodes and carry no weights.
 * Nothing of the context changes (phi, wphi, I, J, Gamma, the rates, its rays, its profile bookkeeping), nothing is created,
 * and only this request crosses to the device.  All pointers are host pointers. */
#define LWHIP_RAYS_MAX_MU 16
typedef struct lwhip_rays {
    int32_t Nmu;            /* 1 .. LWHIP_RAYS_MAX_MU directions                                                    */
    int32_t laStart, laEnd; /* rows [laStart, laEnd) of the GLOBAL wavelength grid, inside the context's own rows
                             * (its shard); 0, 0 = all the context holds.  Nla = laEnd - laStart below             */
    int32_t _pad;
    const double* muz;      /* [Nmu] direction cosines, 0 < mu <= 1                                                 */
    const double* vz;       /* [Nspace] vertical velocity, or NULL: vlosMu[0] / muz[0] of the resident atmosphere
                             * (the 1D convention vlosMu = muz (x) v_z), read on the device                         */
    const double* lowerBc;  /* [Nla, Nmu] intensity entering at the bottom: required with a CALLABLE lower boundary
                             * (which has no data for new directions), ignored otherwise                            */
    double* I;              /* [Nla, Nmu] out: emergent intensity (k = 0)                                           */
    double* depthChi;       /* [Nla, Nmu, Nspace] out or NULL (all three or none): chi, eta and I along each ray,   */
    double* depthEta;       /* what DepthData holds for the to-observer direction                                   */
    double* depthI;
} lwhip_rays;
/* Refusals, before anything is queued: no device LWHIP_ERR_DEVICE; a 2D context, hybrid PRD tables (served by
 * lwhip_compute_rays_hprd below), another formal solver
 * than piecewise_bezier3_1d, Nmu above LWHIP_RAYS_MAX_MU: LWHIP_ERR_UNSUPPORTED; a direction
 * cosine outside (0, 1], a range outside the context's rows, a CALLABLE lower boundary without lowerBc, a line without aDamp,
 * neither vz nor vlosMu, one or two of the three depth arrays: LWHIP_ERR_INVALID.  The call returns when the outputs are
 * in place (one copy back, one wait). */
int lwhip_compute_rays(lwhip_context* ctx, const lwhip_rays* rays);
/* The same for every column of a batch in one launch: perColumn [n], each with its own arrays; Nmu, the wavelength range and
 * the presence of the depth arrays are the same for every column (LWHIP_ERR_INVALID otherwise), the directions, vz and
 * lowerBc may differ.  Each column's results are the bits of lwhip_compute_rays on it. */
int lwhip_batch_compute_rays(lwhip_batch* batch, const lwhip_rays* perColumn);

/* ---- observer rays on a caller-chosen wavelength grid (1D) -----------------------------------------------------------------
 * LwContext.compute_rays(wavelengths, mus) (Source/LwMiddleLayer.pyx:3898-4002) from the state resident on the device: the
 * emergent intensity of lwhip_compute_rays on `wavelength` [Nwave] instead of rows of the context's own grid.  What the reference
 * does for a new grid (lightweaver/atomic_set.py:209-257, LwMiddleLayer.pyx:1960-1963, :2770-2774, :3866):
 *   - active set: with Nb = searchsorted(old grid, wavelength[0]) and Nr = min(searchsorted(old grid, wavelength[Nwave - 1]) + 1,
 *     Nlambda) (both from the left), a transition is active iff its rows [Nblue, Nred) of the old grid meet [Nb, Nr); an active
 *     transition is active on EVERY row of the new grid, an inactive one contributes nothing (lwhip_rays_grid_active);
 *   - J and, for PRD lines, rhoPrd on the new grid: linear interpolation in wavelength per depth point (J from the old grid,
 *     rho from the line's own old grid), the end values held outside, a node hit exactly -- numpy.interp.  Formed on the device
 *     from the RESIDENT J and rho; nothing is downloaded;
 *   - the background and the continuum cross-sections on the new grid come from the model layer: here they are inputs.
 * Then chi, S and the piecewise_bezier3_1d march of lwhip_compute_rays (the same kernel, reading the request's rows).  Nothing of
 * the context changes, nothing is created; the request crosses in one copy, the outputs come back in one.  All pointers are host
 * pointers.  Not served: Stokes, 2D, wavelength shards, a PRD refinement on the new grid; hybrid PRD by
 * lwhip_compute_rays_grid_hprd below. */
typedef struct lwhip_rays_grid {
    lwhip_rays rays;              /* Nmu, muz, vz, I, the depth arrays as for lwhip_compute_rays with Nla = Nwave (lowerBc
                                   * [Nwave, Nmu], I [Nwave, Nmu], depth arrays [Nwave, Nmu, Nspace]); laStart = laEnd = 0 */
    int32_t Nwave, _pad;          /* >= 2                                                                                */
    const double* wavelength;     /* [Nwave] nm, finite and strictly increasing                                          */
    const double* bgChi;          /* [Nwave, Nspace] background opacity, emissivity and scattering on the new grid       */
    const double* bgEta;
    const double* bgSca;
    const double* const* contAlpha; /* [Ntrans_total] in the context's transition order (atoms in order, each atom's
                                   * transitions in order): entry t -> [Nwave] cross-section of an ACTIVE continuum; ignored
                                   * (may be NULL) for lines and inactive transitions; NULL itself if no continuum is active */
} lwhip_rays_grid;
/* The active set of `wavelength` [Nwave] by the rule above: active[t] = 1 / 0 for every transition, in the order of contAlpha.
 * Host work only (no device needed).  A null argument, Nwave < 1: LWHIP_ERR_INVALID. */
int lwhip_rays_grid_active(lwhip_context* ctx, const double* wavelength, int Nwave, int32_t* active);
/* Refusals, before anything is queued and with the outputs untouched: no device LWHIP_ERR_DEVICE; everything
 * lwhip_compute_rays refuses; a wavelength shard (J of the other rows is not resident): LWHIP_ERR_UNSUPPORTED; Nwave < 2, a grid
 * that is not finite or not strictly increasing, a missing background array, a NULL cross-section of an active continuum,
 * laStart or laEnd other than 0: LWHIP_ERR_INVALID. */
int lwhip_compute_rays_grid(lwhip_context* ctx, const lwhip_rays_grid* rays);
/* The same for every column of a batch in one set of launches: perColumn [n]; Nwave, the grid values, Nmu and the presence of the
 * depth arrays are those of column 0 (LWHIP_ERR_INVALID otherwise, the column named); the backgrounds, cross-sections,
 * directions, vz and lowerBc are each column's own.  Each column's results are the bits of lwhip_compute_rays_grid on it. */
int lwhip_batch_compute_rays_grid(lwhip_batch* batch, const lwhip_rays_grid* perColumn);

/* ---- observer rays of a hybrid-PRD context (1D) ------------------------------------------------------------------------------
 * The four calls above refuse a context made with lwhip_options.hprd: rho of a line of its hybrid list (lwhip_hprd.lineAtom /
 * lineTrans) is not the row's.  The reference's second context runs configure_hprd_coeffs on the new rays' vlosMu
 * (LwMiddleLayer.pyx:2822-2826, Prd.cpp:899-939) and Transition::uv interpolates the rest-frame rhoPrd for each ray
 * (LwTransition.hpp:116-127).  These four do that where they gather, as they do phi -- no table is built or stored.  For a line of
 * the hybrid list at its own-grid index lt, direction m and depth k, with w [nlt] the line's own grid:
 *     lambdaRest = w[lt] * (1 + muz[m] v_z[k] / c)
 *     (i0, i1, frac): lambdaRest <= w[0]: (0, 1, 0); lambdaRest >= w[nlt - 1]: (nlt - 2, nlt - 1, 1); else i0 the last node
 *                     <= lambdaRest, i1 = i0 + 1, frac = (lambdaRest - w[i0]) / (w[i1] - w[i0])
 *     rho = (1 - frac) rhoPrd(i0, k) + frac rhoPrd(i1, k),    Vji = (gij Vij) rho
 * every operation rounded once (no fused multiply-add), so the coefficient is the bits of the table entry the reference would
 * hold.  A PRD line outside the hybrid list keeps rho by row.  On a new grid w is the request's grid (nlt = Nwave) and rhoPrd the
 * rho interpolated onto it, which is what the reference's second context holds.
 * Requests, staging, launch shape, outputs and depth arrays are those of the plain calls; nothing of the context changes (I, J,
 * rho, JRest, the tables, phi, the tile lists).  The stored-grid call serves a wavelength shard for its own rows: under hybrid
 * PRD every shard holds rho of each line's whole grid.
 * Refusals, before anything is queued and with the outputs untouched: what the corresponding plain call refuses, except the
 * hybrid tables; a context (or a column, which is named) WITHOUT hybrid tables: LWHIP_ERR_INVALID.
 * Not served: full Stokes, a PRD refinement on the new grid, 2D. */
int lwhip_compute_rays_hprd(lwhip_context* ctx, const lwhip_rays* rays);
int lwhip_batch_compute_rays_hprd(lwhip_batch* batch, const lwhip_rays* perColumn);
int lwhip_compute_rays_grid_hprd(lwhip_context* ctx, const lwhip_rays_grid* rays);
int lwhip_batch_compute_rays_grid_hprd(lwhip_batch* batch, const lwhip_rays_grid* perColumn);

/* ---- full Stokes along observer rays (1D) --------------------------------------------------------------------------------
 * LwContext.compute_rays(mus, stokes=True) (Source/LwMiddleLayer.pyx:3898-4002) from the state resident on the device: for
 * every wavelength of [laStart, laEnd) and every direction the emergent Stokes vector (I, Q, U, V at k = 0) of the up-going
 * ray -- what lwhip_full_stokes_fs(updateJ = 0, upOnly = 1) gives on the context the reference would construct: the same state
 * (n, J, rhoPrd, background), rays muz, vlosMu = mu (x) v_z, wmu = 0, the field projected onto the new directions, the polarised
 * profiles of those directions (Transition::compute_polarised_profiles, Source/FormalStokes.cpp:9-117) and the plain Voigt phi
 * for the other lines.  Needs Stokes data (lwhip_set_stokes): B and the Zeeman components are the resident ones; the profiles
 * are formed inside the gather kernel where it needs them and never stored.  As the reference does, and therefore:
 *   - no scattering term: without updateJ the Stokes source function uses J dagger = 0 (Source/FormalStokes.cpp:429-438, :591;
 *     see lwhip_full_stokes_fs), so at wavelengths with background scattering I here is NOT the I of lwhip_compute_rays;
 *   - a wavelength without a polarised line (and without J20) takes the scalar piecewise_bezier3_1d march and its Q, U, V are
 *     exact zeros, as in lwhip_full_stokes_fs; hasJ20 follows the attached lwhip_stokes descriptor as there;
 *   - any 1D formal solver is accepted: the Stokes path ignores the one the context was built with, so piecewise_linear_1d
 *     and piecewise_besser_1d contexts are served here, unlike lwhip_compute_rays.
 * Nothing of the context changes (I, Quv, J, any line's phi / wphi / phiQ..psiV, its profile bookkeeping, the argument blocks
 * lwhip_full_stokes_fs keeps); only the request crosses to the device and only I and Quv come back (one copy each way, one
 * wait).  All pointers are host pointers. */
typedef struct lwhip_stokes_rays {
    lwhip_rays rays;         /* Nmu, range, muz, vz, lowerBc, I as for lwhip_compute_rays; the three depth arrays must be NULL */
    const double* cosGamma;  /* [Nmu, Nspace] projections of the field on the new directions, computed by the caller */
    const double* cos2chi;   /* (as in lwhip_stokes: Atmosphere::update_projections)                                  */
    const double* sin2chi;
    double* Quv;             /* [3, Nla, Nmu] out */
} lwhip_stokes_rays;
/* Refusals, before anything is queued and with the outputs untouched: no device LWHIP_ERR_DEVICE; what lwhip_full_stokes_fs
 * refuses (2D, a wavelength shard, hybrid PRD tables: LWHIP_ERR_UNSUPPORTED; no Stokes data: LWHIP_ERR_INVALID); what
 * lwhip_compute_rays refuses, except the formal solver; a missing projection array or Quv, a depth array present:
 * LWHIP_ERR_INVALID.  A singular 4 x 4 system: LWHIP_ERR_SINGULAR, the outputs written all the same. */
int lwhip_compute_stokes_rays(lwhip_context* ctx, const lwhip_stokes_rays* rays);
/* The same for every column of a batch in one set of launches: perColumn [n]; the conditions of lwhip_batch_full_stokes_fs (every
 * column with column 0's polarised lines) and of lwhip_batch_compute_rays (Nmu and the wavelength range of column 0), the
 * offending column named.  Each column's results are the bits of lwhip_compute_stokes_rays on it. */
int lwhip_batch_compute_stokes_rays(lwhip_batch* batch, const lwhip_stokes_rays* perColumn);

/* ---- emergent spectra along observer rays (2D) --------------------------------------------------------------------------
 * LwContext.compute_rays(mus, upOnly=True) (Source/LwMiddleLayer.pyx:3898-4002) on a 2D context, from the state resident on the
 * device: for every wavelength of [laStart, laEnd) and every direction (mux[m], muz[m]) the up-going rays through the x-periodic
 * grid, I at the top plane.  The intersection table of the directions is built on the host (lwhip_build_intersections), uploaded
 * and kept until a call asks for other directions; chi and S are gathered as lwhip_formal_sol gathers them, except that each
 * line's profile is evaluated in the kernel: phi = H(aDamp, v) / (sqrt(pi) vBroad), v = ((lambda - lambda0) c / lambda0 +
 * mux vx + muz vz) / vBroad; the solve is the 2D formal solver of lwhip_formal_sol(upOnly).  Nothing of the context changes, and
 * only this request crosses to the device.  All pointers are host pointers.  Nspace = Nz Nx, Nla = laEnd - laStart. */
typedef struct lwhip_rays2d {
    int32_t Nmu;            /* 1 .. LWHIP_RAYS_MAX_MU directions */
    int32_t laStart, laEnd; /* as in lwhip_rays: rows of the GLOBAL grid inside the context's own rows; 0, 0 = all */
    int32_t _pad;
    const double* muz;      /* [Nmu] 0 < muz <= 1 */
    const double* mux;      /* [Nmu] signed; muz^2 + mux^2 <= 1 (the remainder is muy, which a 2D atmosphere never reads) */
    const double* vz;       /* [Nspace] vertical and */
    const double* vx;       /* [Nspace] horizontal velocity: vlos = mux vx + muz vz (Source/Atmosphere.cpp:20-29) */
    const double* lowerBc;  /* [Nla, Nmu, Nx]: required with a CALLABLE z lower boundary, ignored otherwise */
    double* I;              /* [Nla, Nmu, Nx] out: emergent intensity of the up-going rays at the top plane */
} lwhip_rays2d;
/* Refusals, before anything is queued and with I untouched: a null context or request, a missing muz / mux / vz / vx / I, muz
 * outside (0, 1] or muz^2 + mux^2 > 1 + 1e-12, a range outside the context's rows, a CALLABLE lower boundary without lowerBc, a
 * line without aDamp: LWHIP_ERR_INVALID; no device: LWHIP_ERR_DEVICE; a 1D context, a grid with fixed (CALLABLE) x boundaries
 * (they have no data for new directions), Nmu above LWHIP_RAYS_MAX_MU, directions whose table has a long characteristic that
 * does not end on a z plane: LWHIP_ERR_UNSUPPORTED.  The call returns when I is in place (one copy back, one wait). */
int lwhip_compute_rays_2d(lwhip_context* ctx, const lwhip_rays2d* rays);

/* Block until all work queued on the context's stream has finished. */
int lwhip_synchronize(lwhip_context* ctx);

/* ZPlaneDecomposition (ExtraParams "ZPlaneDecomposition" with "ZPlaneDown" / "ZPlaneUp",
 * Source/SimdFullIterationTemplates.hpp:253-281, 351-384): from now on every formal solution also records the
 * intensity of the down rays in plane Nz - 2 (zPlaneDown) and of the up rays in plane 1 (zPlaneUp), host arrays
 * [Nlambda, Nrays] (1D) or [Nlambda, Nrays, Nx] (2D) filled by lwhip_download(LWHIP_I); NULL turns one off. */
int lwhip_set_zplane_outputs(lwhip_context* ctx, double* zPlaneDown, double* zPlaneUp);

/* Use `stream` (hipStream_t) for all subsequent launches; NULL = the library's own. */
int lwhip_set_stream(lwhip_context* ctx, void* stream);

/* Measurement support (bench.py): when enabled, launches of the sweep kernel (raymarch_kernel, the
 * dominant kernel of the iteration; not the pre-pass or the apply launch) are bracketed by HIP events on
 * the launch stream -- every launch for enable = 1, every n-th for enable = n > 1 (two event records
 * cost ~5 us of a 250 us step) -- and lwhip_sweep_time returns the mean duration (ms) and the number
 * of launches timed since the last reset. */
int lwhip_profile_enable(lwhip_context* ctx, int enable);
int lwhip_sweep_time(lwhip_context* ctx, double* meanMs, int* nLaunches);

/* Algorithmic bytes one iteration of this context moves (SURVEY.md 8d / DESIGN.md). */
int lwhip_algorithmic_bytes(lwhip_context* ctx, double* bytes);
/* Which sweep kernel serves this context (chosen at lwhip_create from its size, LWHIP_SWEEP overrides):
 * 0 the ray-column march (raymarch_kernel), 1 the depth-across-lanes sweep (lanesweep_kernel), 2 the 2D pipeline. */
int lwhip_sweep_kind(lwhip_context* ctx);
/* The march on deep columns: the number of wavefronts S a direction's depth points are split over in the
 * main sweep of this context -- 1, 2 or 4, chosen at lwhip_create so that the split launch fits a workgroup's LDS; 1 for
 * the lane sweep and for 2D; -1 for a null context. */
int lwhip_depth_split(lwhip_context* ctx);
/* What a 2D context launches, from the same host functions its launchers call:
 *   out[0], out[1]  fs2d_scan_kernel<D, FULL>: columns per lane (1, 2, 4, 8, 16) and whether Nx = 64 D
 *   out[2]          gather2d_kernel<MAXL>
 *   out[3 .. 5]     rates2d_kernel<MAXL, MAXM, MAXP>
 *   out[6], out[7]  wavelengths per batch, wavelength groups of the rates kernel
 *   out[8]          1: pass 1 reads the packed intersection records, the long characteristics are walked by their own launch
 *   out[9]          NlongChar of the context's grid
 * LWHIP_ERR_UNSUPPORTED for a 1D context, LWHIP_ERR_INVALID for a null argument. */
int lwhip_layout_2d(lwhip_context* ctx, int32_t out[10]);
/* What a 1D context launches, read from the members its launches read; launches nothing, changes nothing:
 *   out[0]          sweep kind: 0 the ray-column march, 1 the depth-across-lanes sweep
 *   out[1 .. 3]     lane sweep: D points per lane, LR lanes per ray, R wavelengths per wavefront (0 on the march)
 *   out[4]          wavefronts per workgroup (tileWaves)
 *   out[5], out[6]  wavefronts a tile's rays are split over in the main sweep / in the PRD rates pass (1 on the march)
 *   out[7]          nTiles
 *   out[8]          1: the two rays of an angle are paired (symmetric profiles of the resident atmosphere, LWHIP_PAIR_RAYS)
 *   out[9]          1: the iso-ray hoist is in force as well (direction-independent profiles, LWHIP_ISO_RAYS)
 * (out[8], out[9]: of a context's own launches; a fused batch launch pairs only if every column does.)
 * LWHIP_ERR_UNSUPPORTED for a 2D context, LWHIP_ERR_INVALID for a null argument. */
int lwhip_layout_1d(lwhip_context* ctx, int32_t out[10]);
/* Which instance of lanesweep_kernel a 1D context's launches take, by the launcher's own rule on the members
 * the launches read; launches nothing, changes nothing.  The plain instance leaves out what a launch does not use -- the depth
 * data stores, the z-plane rows, the CALLABLE boundary lookup; Bezier3 with rates, not hybrid PRD -- and computes the same bits:
 *   out[0]          1: the main sweep of an iteration takes the plain instance
 *   out[1]          1: the PRD rates pass does (it writes no depth data even where the context stores them; 0 without one)
 *   out[2]          1: the depth-across-lanes sweep serves this context (0: the march, which has one instance)
 *   out[3]          the switch LWHIP_LS_PLAIN as read at lwhip_create (0: every launch takes the full instance)
 * LWHIP_ERR_UNSUPPORTED for a 2D context, LWHIP_ERR_INVALID for a null argument.
 * lwhip_batch_sweep_instance: the same of a column batch's one sweep launch, plain only if every column's would be (out[1] = 0). */
int lwhip_sweep_instance(lwhip_context* ctx, int32_t out[4]);
int lwhip_batch_sweep_instance(lwhip_batch* batch, int32_t out[4]);
/* The shape of a column batch's sweep launches; launches nothing, changes nothing.  perColumn [n][2]: each column's workgroup
 * count in the full sweep and in the PRD rates pass (0 without one); launch[0], launch[1]: gridDim.x of the batch's one launch
 * of either for the current active set (launch[1] = 0 on the ray-column march, whose PRD pass is not fused).  Equal for every
 * column except in hybrid-PRD batches, where the launch takes the largest.  LWHIP_ERR_INVALID for a null argument. */
int lwhip_batch_sweep_shape(lwhip_batch* batch, int32_t* perColumn /* [n][2] */, int32_t launch[2]);
/* A fingerprint of what lwhip_create planned for this context; launches nothing, copies nothing:
 *   out[0]          folds the element count and content fingerprint of every structure-table buffer, in the order the
 *                   library lists them (a context made with lwhip_create_like reports its owner's words)
 *   out[1]          folds the scalars of the plan (sweep kind, D / LR / R, tile, chunk and slot counts, splits, totals)
 * Equal words: the same tables and the same launch layout.  They depend on the problem's structure, the options, the
 * environment's layout knobs and the device's compute-unit count.  LWHIP_ERR_INVALID for a null argument. */
int lwhip_tables_signature(lwhip_context* ctx, uint64_t out[2]);

#ifdef __cplusplus
}
#endif
#endif /* LWHIP_H */
