// CFAR, the route of a uint8 call: which kernel it takes, which template instance, and the launch shape -- decided once,
// before the first launch, from a description of the call that holds no pointer.  Plain C++ without a HIP call, so the
// rules can be run on their own (tests/host/cfar_route_check.cpp).  The decision tables the kernels read (CfarLut,
// CfarOsTab, CfarOsGateTab) and the threshold arithmetic (cfar_thr_arith) are here too: whether a table can be built is
// part of the route, and a table is built once per call.
#pragma once

#include <cmath>
#include <cstdint>

#include "../../include/sonarfe.h"

#if defined(__HIPCC__)
#define SFE_CFAR_HD __host__ __device__ __forceinline__
#else
#define SFE_CFAR_HD static inline
#endif

// ---------------------------------------------------------------------------------------------------------------------
// The reference's threshold of a window sum s (cfar.cpp:27,46,67): tau * s / T, with / (2 T) for CA; s is held in a float.
// ---------------------------------------------------------------------------------------------------------------------
static inline double cfar_divisor(int alg, int T) { return alg == SFE_CFAR_CA ? 2.0 * T : (double)T; }
static inline double cfar_ref_thr(int alg, int T, double tau, long long s)
{
    return tau * (double)(float)s / cfar_divisor(alg, T);
}
// the largest window sum of uint8 pixels
static inline long long cfar_smax(int alg, int T) { return 255ll * (alg == SFE_CFAR_CA ? 2ll * T : (long long)T); }

// lut[x] = #{s : x > thr(s)}: the pixel fires iff its window sum s < lut[x] (the decision is monotone in s)
struct CfarLut {
    uint16_t v[256];
};
// false: no table for this call (tau negative or not finite, sums beyond 16 bits)
static inline bool build_lut(int alg, int T, double tau, int intensity_thr, CfarLut *lut)
{
    if (!(tau >= 0.0) || !std::isfinite(tau))
        return false;
    const long long smax = cfar_smax(alg, T);
    if (smax + 1 > 65535)
        return false;
    for (int x = 0; x < 256; ++x) {
        int cnt = 0;
        if (!(intensity_thr >= 0 && x <= intensity_thr) && (double)(float)x > cfar_ref_thr(alg, T, tau, 0)) {
            int lo = 0, hi = (int)smax; // s = lo passes; find the largest passing s (monotone in s)
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if ((double)(float)x > cfar_ref_thr(alg, T, tau, mid))
                    lo = mid;
                else
                    hi = mid - 1;
            }
            cnt = lo + 1;
        }
        lut->v[x] = (uint16_t)cnt;
    }
    return true;
}

// The threshold map's value for a window sum s, thr = (float)cfar_ref_thr(s), computed instead of fetched: one table gather
// per pixel is one L1 tag look-up per pixel, and that rate -- not HBM -- bounded the map kernels (0.47-0.60 ms per 512
// frames whatever the window).  The quotient is formed with the reciprocal of D = T or 2T and two residual corrections
// (fma), which is the correctly rounded quotient for every operand the host has tried: cfar_thr_arith_check evaluates this
// very sequence for every possible sum of the launch and compares it with cfar_ref_thr bit by bit -- a single difference
// and the kernel keeps the table (ta.on = 0).
struct CfarThrArith {
    double tau, rinv, d;
    int on;
};
SFE_CFAR_HD float cfar_thr_arith(const CfarThrArith &ta, uint32_t sv)
{
    const double p = ta.tau * (double)(float)sv;
    double q = p * ta.rinv;
    double e = fma(-ta.d, q, p);
    q = fma(e, ta.rinv, q);
    e = fma(-ta.d, q, p);
    q = fma(e, ta.rinv, q);
    return (float)q;
}
static inline CfarThrArith cfar_thr_arith_of(int alg, int T, double tau, int on)
{
    const double d = cfar_divisor(alg, T);
    return CfarThrArith{tau, 1.0 / d, d, on};
}
// 1 when cfar_thr_arith agrees bit by bit with the reference expression for every window sum of (alg, T, tau)
static inline int cfar_thr_arith_check(int alg, int T, double tau)
{
    const CfarThrArith ta = cfar_thr_arith_of(alg, T, tau, 1);
    const long long smax = cfar_smax(alg, T);
    for (long long sv = 0; sv <= smax; ++sv) {
        const float want = (float)cfar_ref_thr(alg, T, tau, sv);
        const float got = cfar_thr_arith(ta, (uint32_t)sv);
        if (__builtin_memcmp(&want, &got, sizeof want) != 0)
            return 0; // (never seen: the kernels then read the table)
    }
    return 1;
}

// OS, sliding histogram: decision and threshold per order statistic v, in the reference's double expression
struct CfarOsTab {
    uint16_t min_x[256]; // pixel fires iff x >= min_x[v]  (256 = never); the intensity gate is folded in
    float thr[256];      // (float)(tau * v)
};
static inline CfarOsTab cfar_os_tab(double tau, int intensity_thr)
{
    CfarOsTab tab;
    for (int v = 0; v < 256; ++v) {
        const double t = tau * (double)(float)v; // cfar.cpp:92 / :186
        tab.thr[v] = (float)t;
        int mx = 256;
        for (int x = 255; x >= 0; --x) // (double)x > t is monotone in x
            if ((double)(float)x > t && !(intensity_thr >= 0 && x <= intensity_thr))
                mx = x;
            else
                break;
        tab.min_x[v] = (uint16_t)mx;
    }
    return tab;
}

// OS, candidates only (cfar_u8_os_gated): a workgroup stages a tile of OSG_TR x OSG_TC pixels with its window halo
#define OSG_TR 128 // tile rows
#define OSG_TC 128 // tile columns (bytes per staged row)
#define OSG_LIST 192 // candidates a wave collects before it takes 64 of them

struct CfarOsGateTab {
    int16_t L[256]; // pixel value x -> largest v with x > tau * v and x above the gate; -1: never fires
    int xc;         // smallest x with L[x] >= 0 (L grows with x: "can fire at all" is one threshold); 257: none
    // PREF (no gate, or a low one: round 6): the level l0 of the pre-filter and what the kernel needs of it
    int x_hi;       // smallest x with L[x] > l0 (257: none)
    int c0;         // l0 + 1: a training cell counts as "above" when it is >= c0
    int m_le;       // 2T - (k + 1): at most that many cells above l0 <=> at least k + 1 cells <= l0
};
struct CfarOsGate {
    CfarOsGateTab tab;
    bool applies; // pref: false when there is no level to filter on or the packed counters do not hold the window
};
// pref: the pre-filtered form for a missing or low gate (see the kernel), with its level taken at pixel value pref_x
static inline CfarOsGate cfar_os_gate_tab(int T, int k, double tau, int intensity_thr, bool pref, int pref_x)
{
    CfarOsGate g;
    CfarOsGateTab &tab = g.tab;
    for (int x = 0; x < 256; ++x) {
        int L = -1;
        if (!(intensity_thr >= 0 && x <= intensity_thr))
            for (int v = 0; v < 256; ++v) { // (double)x > tau * v is monotone in v: the largest v that still holds
                const double t = tau * (double)(float)v; // cfar.cpp:92
                if ((double)(float)x > t)
                    L = v;
                else
                    break;
            }
        tab.L[x] = (int16_t)L;
    }
    tab.xc = 257;
    for (int x = 255; x >= 0; --x)
        if (tab.L[x] >= 0)
            tab.xc = x;
    tab.x_hi = 257;
    tab.c0 = 1;
    tab.m_le = 0;
    g.applies = true;
    if (pref) {
        // the level: what a pixel of a third of full scale is compared with (L[80]; tuning cfar_os_pref_x moves it).  Any
        // level is exact; this one keeps both kinds of candidates rare on sonar images
        const int xs = tab.xc > pref_x ? tab.xc : pref_x;
        const int l0 = xs <= 255 ? tab.L[xs] : -1;
        g.applies = l0 >= 0 && l0 < 255 && 2 * T <= 127 && k + 1 <= 2 * T;
        if (g.applies) {
            tab.c0 = l0 + 1;
            tab.m_le = 2 * T - (k + 1);
            for (int x = 255; x >= 0; --x)
                if (tab.L[x] > l0)
                    tab.x_hi = x;
        }
    }
    return g;
}

// ---------------------------------------------------------------------------------------------------------------------
// The call
// ---------------------------------------------------------------------------------------------------------------------
enum CfarOut { CFAR_OUT_MASK, CFAR_OUT_BITS, CFAR_OUT_MASK_THR }; // byte mask / bit stream / byte mask + float threshold map

// the alignment of an address as the rules ask for it: 0 = null, else the largest of 1, 2, 4, 8, 16 that divides it
static inline int cfar_align_of(const void *p)
{
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    return !a ? 0 : (int)((a | 16) & (~(a | 16) + 1));
}

struct CfarCall {
    int rows, cols, n_frames, alg, T, G, k;
    double tau;
    int intensity_thr;
    int img_align, out_align, thr_align; // cfar_align_of the image, the mask or bit stream, the threshold map
    CfarOut out;
    int variant, tile_rows;                             // sfe_cfar_set_tuning
    int os_gated, os_gated_min, os_pref, os_pref_x;     // sfe_tune cfar_os_*
    int thr_arith_on;                                   // cfar_thr_arith_check(alg, T, tau), for a call with a threshold map
};

// ---------------------------------------------------------------------------------------------------------------------
// The route.  A call is refused (bad argument, or the ring kernel forced where it does not apply), has nothing to do, or
// takes exactly one kernel:
//
//   route        kernel                        taken when
//   RING         cfar_u8_ring<T,G,ALG,D,..>    CA/SOCA/GOCA, a compiled window (CFAR_RING_WINDOWS), rows >= R = 2(T+G)+2,
//                                              cols >= 256, `aligned`, the LUT exists, variant != 1; with a threshold map
//                                              also cfar_thr_arith checked out.  Bit stream: cols % 32 == 0 and variant 0
//   PACK         (bit-stream call only)        the bit-stream ring does not apply: the byte kernels below into scratch, a
//                                              bounded number of frames at a time, each followed by mask_pack
//   SLIDE_LDS    cfar_u8_slide_lds<ALG,THR>    CA/SOCA/GOCA, not RING, `aligned`, the LUT exists, variant != 1, R <= 80
//   SLIDE        cfar_u8_slide<ALG,THR>        the same with R > 80 rows
//   OS_GATED     cfar_u8_os_gated<V16,0>       OS, 2T <= 255, pixels < 2^30, variant != 1, no threshold map, `aligned`, the
//                                              tile fits the LDS limit, cfar_os_gated and gate >= cfar_os_gated_min
//   OS_PREF      cfar_u8_os_gated<V16,1|2>     the same without such a gate, cfar_os_pref, and the pre-filter applies
//                                              (a level l0 < 255 exists, 2T <= 127)
//   OS_HIST      cfar_u8_os                    OS, 2T <= 255, pixels < 2^30, variant != 1, none of the two above
//   GENERIC      cfar_u8_generic               everything else: odd widths, unaligned buffers, no LUT, variant 1, 2T > 255
//
//   `aligned`: cols % 4 == 0, pixels < 2^30, image and output 4-byte aligned, the threshold map (if any) 16-byte aligned.
//   Variants 2 and 3 force RING: a mask call that would take another route is refused.
// ---------------------------------------------------------------------------------------------------------------------
enum CfarKernel {
    CFAR_NONE, // nothing to do, or refused
    CFAR_PACK,
    CFAR_RING,
    CFAR_SLIDE_LDS,
    CFAR_SLIDE,
    CFAR_OS_GATED,
    CFAR_OS_PREF,
    CFAR_OS_HIST,
    CFAR_GENERIC
};

// register-ring kernel: instantiated for the shipped window (Ntc 40, Ngc 10 -> 20, 5) and for the other windows the
// reference's feature.yaml comments and tests go through: (32, 8), (20, 4), (16, 2).  X(T, G, D): D = rows in flight
// (prefetch depth, divides R).  Variant 3 runs the shipped window with D = 13 (byte mask only): the last instance.
#define CFAR_RING_WINDOW_LIST(X) X(20, 5, 4) X(16, 4, 6) X(10, 2, 13) X(8, 1, 5)
#define CFAR_RING_V3(X) X(20, 5, 13)
struct CfarRingWindow {
    int T, G, D;
};
#define CFAR_RING_ENTRY(T, G, D) {T, G, D},
static const CfarRingWindow CFAR_RING_WINDOWS[] = {CFAR_RING_WINDOW_LIST(CFAR_RING_ENTRY) CFAR_RING_V3(CFAR_RING_ENTRY)};
#undef CFAR_RING_ENTRY
static const int CFAR_RING_INSTANCES = (int)(sizeof(CFAR_RING_WINDOWS) / sizeof(CFAR_RING_WINDOWS[0]));
static const int CFAR_RING_V3_INSTANCE = CFAR_RING_INSTANCES - 1;

struct CfarRoute {
    const char *refusal = nullptr; // the argument condition that fails (SFE_ERR_ARG "bad argument: ...")
    bool ring_forced = false;      // variant 2 / 3 on a call the ring kernel does not take (SFE_ERR_ARG)
    CfarKernel kernel = CFAR_NONE;
    // instance: RING an index into CFAR_RING_WINDOWS; OS_GATED / OS_PREF the kernel's PREF (0, 1, 2) with v16
    int instance = 0, v16 = 0;
    // launch shape: RING groups (R-row groups per tile), tiles, chunks; SLIDE* tile_rows, tiles, chunks; OS_GATED / OS_PREF
    // tiles (rows of tiles), chunks (columns of tiles); OS_HIST and GENERIC tile_rows, tiles, chunks (GENERIC: none)
    int groups = 0, tile_rows = 0, tiles = 0, chunks = 0;
    long long workgroups = 0, out_frame_bytes = 0;
    long long lds_bytes = 0; // dynamic LDS
    CfarLut lut = {};        // RING, SLIDE*
    CfarThrArith ta = {0.0, 0.0, 1.0, 0};
    CfarOsTab os_tab = {};   // OS_HIST
    CfarOsGateTab gate_tab = {}; // OS_GATED, OS_PREF
};

static inline int cfar_ring_rows(int T, int G) { return 2 * (T + G) + 2; } // R: the rows a window spans, + 2

static inline bool cfar_aligned(const CfarCall &c)
{
    return c.cols % 4 == 0 && (long long)c.rows * c.cols < (1ll << 30) && c.img_align >= 4 && c.out_align >= 4 &&
           (c.out != CFAR_OUT_MASK_THR || c.thr_align >= 16);
}

// index into CFAR_RING_WINDOWS of the instance this call takes if the ring kernel takes it, else -1.  The bit-stream form
// differs in two places: whole 32-bit words per row, and no tuning variant (BITS is compiled for the default depth only)
static inline int cfar_ring_instance(const CfarCall &c)
{
    const bool bits = c.out == CFAR_OUT_BITS;
    if (c.alg == SFE_CFAR_OS || !cfar_aligned(c) || c.cols < 256 || c.rows < cfar_ring_rows(c.T, c.G) ||
        c.cols % (bits ? 32 : 4) != 0 || (bits ? c.variant != 0 : c.variant == 1))
        return -1;
    // (with a threshold map: when it can be computed, cfar_thr_arith)
    if (c.out == CFAR_OUT_MASK_THR && !c.thr_arith_on)
        return -1;
    if (c.out == CFAR_OUT_MASK && c.variant == 3 && c.T == CFAR_RING_WINDOWS[CFAR_RING_V3_INSTANCE].T &&
        c.G == CFAR_RING_WINDOWS[CFAR_RING_V3_INSTANCE].G)
        return CFAR_RING_V3_INSTANCE;
    for (int i = 0; i < CFAR_RING_V3_INSTANCE; ++i)
        if (c.T == CFAR_RING_WINDOWS[i].T && c.G == CFAR_RING_WINDOWS[i].G)
            return i;
    return -1;
}

// R-row groups per tile.  Measured on MI355X (tools/cfar_sweep.py, 1024 frames of 1024x512, XCD-aware
// map + alternating march direction):  1 group/tile 5.1 TB/s with FETCH = 1.30x the image bytes,
// 2 groups 5.1 TB/s with 1.13x, 4 groups 4.9 TB/s with 1.07x, whole column 3.1 TB/s.  Short tiles win
// on time (the kernel is bound by each wave's serial row march, more independent waves hide it);
// 2 groups keep that speed and most of the 2*(T+G) halo rows a tile re-reads are L2 hits.
static inline int default_groups(int rows, int R) { return rows >= 2 * R ? 2 : 1; }

static inline long long cfar_ceil_div(long long a, long long b) { return (a + b - 1) / b; }
// RING and SLIDE*: four waves of a workgroup take four (tile, chunk) pairs; frames padded to the 8 XCDs
static inline long long cfar_wave_workgroups(int n_frames, int tiles, int chunks)
{
    return cfar_ceil_div(n_frames, 8) * 8 * cfar_ceil_div((long long)tiles * chunks, 4);
}
// the staged tile of cfar_u8_os_gated must leave room for a second workgroup on the CU
static inline bool cfar_osg_fits(int T, int G) { return (long long)(OSG_TR + 2 * (T + G)) * OSG_TC <= 96 * 1024; }

static inline CfarRoute cfar_route(const CfarCall &c)
{
    CfarRoute r;
    // the argument refusals
    if (!(c.img_align && c.out_align))
        r.refusal = "d_img && d_mask";
    else if (!(c.n_frames >= 0 && c.rows >= 0 && c.cols >= 0))
        r.refusal = "n_frames >= 0 && rows >= 0 && cols >= 0";
    else if (!(c.alg >= SFE_CFAR_CA && c.alg <= SFE_CFAR_OS))
        r.refusal = "alg >= SFE_CFAR_CA && alg <= SFE_CFAR_OS";
    else if (!(c.T >= 1 && c.G >= 0))
        r.refusal = "T >= 1 && G >= 0";
    else if (c.alg == SFE_CFAR_OS && !(c.k >= 0 && c.k < 2 * c.T))
        r.refusal = "k >= 0 && k < 2 * T";
    if (r.refusal || c.n_frames == 0 || c.rows == 0 || c.cols == 0)
        return r;
    const int T = c.T, G = c.G, rows = c.rows, cols = c.cols, R = cfar_ring_rows(T, G);
    const bool thr = c.out == CFAR_OUT_MASK_THR, os = c.alg == SFE_CFAR_OS, aligned = cfar_aligned(c);
    const long long px = (long long)rows * cols;
    if (thr && !os)
        r.ta = cfar_thr_arith_of(c.alg, T, c.tau, c.thr_arith_on);
    // CA / SOCA / GOCA: the LUT kernels, ring before slide
    const int ring = cfar_ring_instance(c);
    const bool lut = !os && aligned && c.variant != 1 && (ring >= 0 || c.out != CFAR_OUT_BITS) &&
                     build_lut(c.alg, T, c.tau, c.intensity_thr, &r.lut);
    if (lut && ring >= 0) {
        r.kernel = CFAR_RING;
        r.instance = ring;
        r.groups = c.tile_rows > 0 ? c.tile_rows / R : T == 20 ? default_groups(rows, R) : 104 / R; // ~104-row tiles
        r.groups = r.groups < rows / R ? r.groups : rows / R;
        r.groups = r.groups > 1 ? r.groups : 1;
        r.tiles = (int)cfar_ceil_div(rows, (long long)r.groups * R);
        r.chunks = ((cols >> 2) + 63) / 64;
        r.workgroups = cfar_wave_workgroups(c.n_frames, r.tiles, r.chunks);
        // bytes per frame of the bit stream: one pad word (sfe_extract.hip)
        r.out_frame_bytes = c.out == CFAR_OUT_BITS ? (px / 32 + 1) * 4 : px;
    } else if (c.out == CFAR_OUT_BITS) {
        r.kernel = CFAR_PACK;
    } else if (c.variant >= 2) {
        r.ring_forced = true;
    } else if (lut) {
        // every other window / the threshold maps: sliding sums over a run-time window.  Long tiles: a tile starts with 2T
        // loads per lane to build its first windows
        r.tile_rows = rows < (128 > 8 * T ? 128 : 8 * T) ? rows : (128 > 8 * T ? 128 : 8 * T);
        r.tiles = (int)cfar_ceil_div(rows, r.tile_rows);
        r.chunks = ((cols >> 2) + 63) / 64;
        r.workgroups = cfar_wave_workgroups(c.n_frames, r.tiles, r.chunks);
        // window rows staged in LDS (R KiB per workgroup) unless the window is too tall for it: beyond two workgroups per
        // CU (R > 80 rows = 80 KiB) the ring starves the CU of waves and re-reading the four rows through the caches is
        // faster (measured (80, 20): 15 % of HBM with the LDS ring, 25 % without)
        r.kernel = (long long)R * 1024 <= 80 * 1024 ? CFAR_SLIDE_LDS : CFAR_SLIDE;
        r.lds_bytes = r.kernel == CFAR_SLIDE_LDS ? (long long)R * 1024 : 0;
    } else if (os && c.variant != 1 && 2 * T <= 255 && px < (1ll << 30)) {
        // OS behind a gate: only the pixels above it are looked at (cfar_u8_os_gated).  It pays when the gate removes most
        // pixels -- measured on 512 sonar frames, (Ntc 40, Ngc 10, k 10): gate 65 0.65 ms against the histogram kernel's
        // 1.65 ms; gate 20 (four pixels in ten pass) 1.84 against 1.65 -- so a low gate keeps the histogram kernel
        // (feature.yaml ships 65; tuning cfar_os_gated_min moves the limit).  No gate, or a low one: the pre-filtered
        // candidate kernel (round 6) where it applies, else the sliding histogram
        const bool candidates = !thr && aligned && cfar_osg_fits(T, G);
        const bool gated = candidates && c.os_gated && c.intensity_thr >= c.os_gated_min;
        CfarOsGate g;
        g.applies = false;
        if (gated || (candidates && c.os_pref))
            g = cfar_os_gate_tab(T, c.k, c.tau, c.intensity_thr, !gated, c.os_pref_x);
        if (g.applies) {
            r.kernel = gated ? CFAR_OS_GATED : CFAR_OS_PREF;
            r.gate_tab = g.tab;
            r.instance = gated ? 0 : T == 20 ? 2 : 1;
            r.v16 = cols % 16 == 0 && c.img_align >= 16 && c.out_align >= 16;
            r.tiles = (int)cfar_ceil_div(rows, OSG_TR);
            r.chunks = (int)cfar_ceil_div(cols, OSG_TC);
            r.workgroups = (long long)c.n_frames * r.tiles * r.chunks;
            r.lds_bytes = (long long)(OSG_TR + 2 * (T + G)) * OSG_TC + (long long)OSG_TR * (OSG_TC / 8) +
                          (long long)sizeof(unsigned short) * 4 * (OSG_LIST + 256) + (gated ? 0 : 8 * 32 * 2 * 4);
        } else {
            r.kernel = CFAR_OS_HIST;
            r.os_tab = cfar_os_tab(c.tau, c.intensity_thr);
            r.tile_rows = rows < (256 > 8 * T ? 256 : 8 * T) ? rows : (256 > 8 * T ? 256 : 8 * T);
            r.tiles = (int)cfar_ceil_div(rows, r.tile_rows);
            r.chunks = (cols + 63) / 64;
            r.workgroups = (long long)c.n_frames * r.tiles * r.chunks;
        }
    } else {
        // what is left (odd widths, unaligned buffers, windows beyond the 16-bit sums): one thread per column of a tile
        r.kernel = CFAR_GENERIC;
        r.tile_rows = rows < 64 ? rows : 64;
        r.tiles = (int)cfar_ceil_div(rows, r.tile_rows);
        r.workgroups = cfar_ceil_div((long long)c.n_frames * r.tiles * cols, 256);
    }
    return r;
}
