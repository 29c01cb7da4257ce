// Stand-alone check of the CFAR route (sonar_slam_amd/csrc/sfe_cfar_route.h), run on the CPU.
// tests/test_cfar_route_rules.py builds it plainly; under the sanitizers it is a program of its own (no GPU, nothing
// preloaded):
//   g++ -std=c++17 -O1 -g -Wall -Wextra -Werror -fsanitize=address,undefined -fno-sanitize-recover=all
//       tests/host/cfar_route_check.cpp -o cfar_route_check && ./cfar_route_check [CALLS.txt]
//
// CALLS.txt (written by the test from tests/golden/cfar_routes.json): one call per line with the launches that the kernel
// trace of the commit before this header showed for it.  cfar_route must name the same kernel, the same template
// instance and the same number of workgroups; the dynamic LDS bytes, which the trace does not show, must equal the
// former launch code's formulas, restated here.
//
// Without a file, and before it: the invariants the kernels rely on, over
//   rows 1..300 at cols {8, 37, 256, 260, 288, 600} and cols 1..600 at rows {7, 52, 105, 300};
//   CA, SOCA, GOCA, OS; the ring windows, (12,3), (30,9), (30,10), (64,2), (128,1), (129,1), (130,0);
//   byte mask, bit stream, mask + threshold map; variants 0-3; 1..9 frames; and every alignment of the three buffers on
//   three shapes.
//   * exactly one of: refused / ring forced / one kernel;
//   * RING only for a window of CFAR_RING_WINDOWS, rows >= R, cols >= 256, cols % 4 == 0, pixels < 2^30, 4-byte aligned
//     buffers (16 for the map); the bit-stream form only with cols % 32 == 0 and variant 0; D = 13 only for variant 3;
//   * groups >= 1, groups * R <= rows (the last tile is shifted up, not cut) and tiles * groups * R >= rows;
//   * RING / SLIDE: 4 * workgroups cover tiles * chunks of ceil(n_frames / 8) * 8 frames, 256 * chunks >= cols;
//   * SLIDE_LDS bytes = R KiB <= 80 KiB; SLIDE has none;
//   * OS_GATED / OS_PREF bytes = the former formula, <= 160 KiB, and the tiles cover the image;
//   * the LUT of a RING / SLIDE route is the LUT of the call (so build_lut succeeded);
//   * no int overflow in the workgroup count for 4096 frames of 2048 x 1024;
//   * the 2^30-pixel limit, against expectations written by hand from the former condition
//     `(size_t)rows * cols < (1u << 30)`;
//   * cfar_thr_arith == cfar_ref_thr bit by bit for every window sum of the windows and taus of
//     tests/test_cfar_thr_arith.py.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>

#include "../../sonar_slam_amd/csrc/sfe_cfar_route.h"

static CfarCall g_c;
static const char *g_what = "";

#define CHECK(cond)                                                                                                    \
    do {                                                                                                               \
        if (!(cond)) {                                                                                                 \
            std::fprintf(stderr,                                                                                       \
                         "cfar_route_check: %s fails (line %d) %s: %d frames %d x %d alg %d (%d,%d) k %d tau %g gate " \
                         "%d out %d align %d/%d/%d variant %d tile_rows %d\n",                                        \
                         #cond, __LINE__, g_what, g_c.n_frames, g_c.rows, g_c.cols, g_c.alg, g_c.T, g_c.G, g_c.k,      \
                         g_c.tau, g_c.intensity_thr, (int)g_c.out, g_c.img_align, g_c.out_align, g_c.thr_align,        \
                         g_c.variant, g_c.tile_rows);                                                                  \
            std::exit(1);                                                                                              \
        }                                                                                                              \
    } while (0)

static CfarCall make(int n, int rows, int cols, int alg, int T, int G, CfarOut out, int variant)
{
    CfarCall c;
    c.rows = rows, c.cols = cols, c.n_frames = n, c.alg = alg, c.T = T, c.G = G, c.k = 4;
    c.tau = alg == SFE_CFAR_OS ? 1.2 : 1.1, c.intensity_thr = -1;
    c.img_align = c.out_align = 16, c.thr_align = out == CFAR_OUT_MASK_THR ? 16 : 0;
    c.out = out, c.variant = variant, c.tile_rows = 0;
    c.os_gated = 1, c.os_gated_min = 40, c.os_pref = 1, c.os_pref_x = 80;
    c.thr_arith_on = out == CFAR_OUT_MASK_THR && alg != SFE_CFAR_OS;
    return c;
}

// the former launch code's dynamic LDS of cfar_u8_os_gated
static long long osg_bytes(int T, int G, bool pref)
{
    return (long long)(128 + 2 * (T + G)) * 128 + 128 * (128 / 8) + 2 * 4 * (192 + 256) + (pref ? 8 * 32 * 2 * 4 : 0);
}

static long long g_routes[CFAR_GENERIC + 1], g_refused, g_forced;

static CfarRoute checked_route(const CfarCall &c, const CfarLut *lut)
{
    g_c = c;
    const CfarRoute r = cfar_route(c);
    const int R = 2 * (c.T + c.G) + 2;
    const long long px = (long long)c.rows * c.cols;
    CHECK((r.refusal != nullptr) + r.ring_forced + (r.kernel != CFAR_NONE) == 1);
    g_refused += r.refusal != nullptr, g_forced += r.ring_forced, g_routes[r.kernel]++;
    CHECK(r.kernel == CFAR_NONE || (r.kernel == CFAR_PACK) == (c.out == CFAR_OUT_BITS && r.kernel != CFAR_RING));
    CHECK(!(c.variant >= 2 && c.out != CFAR_OUT_BITS) || r.kernel == CFAR_RING || r.kernel == CFAR_NONE);
    if (r.kernel != CFAR_NONE && r.kernel != CFAR_PACK)
        CHECK(r.workgroups >= 1 && r.workgroups <= INT_MAX);
    const bool lut_kernel = r.kernel == CFAR_RING || r.kernel == CFAR_SLIDE || r.kernel == CFAR_SLIDE_LDS;
    if (lut_kernel) {
        CHECK(c.alg != SFE_CFAR_OS && c.cols % 4 == 0 && px < (1ll << 30) && c.img_align >= 4 && c.out_align >= 4);
        CHECK(c.out != CFAR_OUT_MASK_THR || c.thr_align >= 16);
        CHECK(c.variant != 1);
        CHECK(lut && std::memcmp(&r.lut, lut, sizeof *lut) == 0);
        const long long f8 = (long long)(c.n_frames + 7) / 8 * 8, per_frame = r.workgroups / f8, pairs = (long long)r.tiles * r.chunks;
        CHECK(r.workgroups % f8 == 0 && 4 * per_frame >= pairs && 4 * (per_frame - 1) < pairs);
        CHECK(r.chunks >= 1 && 256 * r.chunks >= c.cols && 256 * (r.chunks - 1) < c.cols);
        CHECK(r.ta.on == (c.out == CFAR_OUT_MASK_THR ? c.thr_arith_on : 0));
    }
    if (r.kernel == CFAR_RING) {
        CHECK(r.instance >= 0 && r.instance < CFAR_RING_INSTANCES);
        const CfarRingWindow w = CFAR_RING_WINDOWS[r.instance];
        CHECK(w.T == c.T && w.G == c.G && R % w.D == 0);
        CHECK((r.instance == CFAR_RING_V3_INSTANCE) == (c.variant == 3 && c.out == CFAR_OUT_MASK && c.T == 20));
        CHECK(c.rows >= R && c.cols >= 256);
        CHECK(c.out != CFAR_OUT_BITS || (c.cols % 32 == 0 && c.variant == 0));
        CHECK(c.out != CFAR_OUT_MASK_THR || c.thr_arith_on);
        CHECK(r.groups >= 1 && (long long)r.groups * R <= c.rows && (long long)r.tiles * r.groups * R >= c.rows);
        CHECK((long long)(r.tiles - 1) * r.groups * R < c.rows);
        CHECK(r.out_frame_bytes == (c.out == CFAR_OUT_BITS ? (px / 32 + 1) * 4 : px) && r.lds_bytes == 0);
    } else if (r.kernel == CFAR_SLIDE || r.kernel == CFAR_SLIDE_LDS) {
        CHECK(c.out != CFAR_OUT_BITS);
        CHECK(r.tile_rows >= 1 && (long long)r.tiles * r.tile_rows >= c.rows && (long long)(r.tiles - 1) * r.tile_rows < c.rows);
        CHECK(r.lds_bytes == (r.kernel == CFAR_SLIDE_LDS ? R * 1024ll : 0) && r.lds_bytes <= 80 * 1024);
        CHECK((r.kernel == CFAR_SLIDE) == (R > 80));
    } else if (r.kernel == CFAR_OS_GATED || r.kernel == CFAR_OS_PREF) {
        const bool pref = r.kernel == CFAR_OS_PREF;
        CHECK(c.alg == SFE_CFAR_OS && c.out == CFAR_OUT_MASK && c.variant == 0 && px < (1ll << 30));
        CHECK(c.cols % 4 == 0 && c.img_align >= 4 && c.out_align >= 4);
        CHECK(pref ? (2 * c.T <= 127 && r.instance == (c.T == 20 ? 2 : 1)) : (2 * c.T <= 255 && r.instance == 0));
        CHECK(r.v16 == (c.cols % 16 == 0 && c.img_align >= 16 && c.out_align >= 16));
        CHECK(r.lds_bytes == osg_bytes(c.T, c.G, pref) && r.lds_bytes <= 160 * 1024);
        CHECK(128ll * r.tiles >= c.rows && 128ll * r.chunks >= c.cols && r.workgroups == (long long)c.n_frames * r.tiles * r.chunks);
        CHECK(pref ? (r.gate_tab.c0 >= 1 && r.gate_tab.c0 <= 255 && r.gate_tab.m_le == 2 * c.T - (c.k + 1)) : r.gate_tab.c0 == 1);
    } else if (r.kernel == CFAR_OS_HIST) {
        CHECK(c.alg == SFE_CFAR_OS && c.out != CFAR_OUT_BITS && c.variant == 0 && 2 * c.T <= 255 && px < (1ll << 30));
        CHECK((long long)r.tiles * r.tile_rows >= c.rows && 64ll * r.chunks >= c.cols);
        CHECK(r.workgroups == (long long)c.n_frames * r.tiles * r.chunks);
    } else if (r.kernel == CFAR_GENERIC) {
        CHECK(c.out != CFAR_OUT_BITS && c.variant <= 1);
        CHECK((long long)r.tiles * r.tile_rows >= c.rows && r.tile_rows <= 64);
        CHECK(256 * r.workgroups >= (long long)c.n_frames * r.tiles * c.cols);
    }
    return r;
}

static const int WINDOWS[][2] = {{20, 5}, {16, 4}, {10, 2}, {8, 1}, {12, 3}, {30, 9}, {30, 10}, {64, 2}, {128, 1}, {129, 1}, {130, 0}};

static void sweep_shape(int rows, int cols, const int (&w)[2], int alg, const CfarLut *lut)
{
    const int n = 1 + (rows + cols) % 9;
    for (int out = 0; out < 3; ++out)
        for (int variant = 0; variant < 4; ++variant)
            for (int gate = -1; gate <= (alg == SFE_CFAR_OS ? 65 : -1); gate += 66) { // OS: without and behind a gate
                CfarCall c = make(n, rows, cols, alg, w[0], w[1], (CfarOut)out, variant);
                c.intensity_thr = gate;
                checked_route(c, lut);
            }
}

static void invariants()
{
    g_what = "grid";
    static const int COLS[] = {8, 37, 256, 260, 288, 600}, ROWS[] = {7, 52, 105, 300}, SHAPES[][2] = {{52, 256}, {140, 64}, {100, 64}};
    static const int ALIGN[] = {16, 8, 4, 2, 1};
    for (const auto &w : WINDOWS)
        for (int alg = SFE_CFAR_CA; alg <= SFE_CFAR_OS; ++alg) {
            CfarLut lut;
            const CfarCall proto = make(1, 1, 1, alg, w[0], w[1], CFAR_OUT_MASK, 0);
            const bool has_lut = alg != SFE_CFAR_OS && build_lut(alg, w[0], proto.tau, proto.intensity_thr, &lut);
            CHECK(has_lut == (alg != SFE_CFAR_OS && cfar_smax(alg, w[0]) + 1 <= 65535));
            for (int rows = 1; rows <= 300; ++rows)
                for (int cols : COLS)
                    sweep_shape(rows, cols, w, alg, has_lut ? &lut : nullptr);
            for (int cols = 1; cols <= 600; ++cols)
                for (int rows : ROWS)
                    sweep_shape(rows, cols, w, alg, has_lut ? &lut : nullptr);
            g_what = "alignments";
            for (const auto &s : SHAPES)
                for (int ia : ALIGN)
                    for (int oa : ALIGN)
                        for (int ta : ALIGN)
                            for (int out = 0; out < 3; ++out) {
                                CfarCall c = make(2, s[0], s[1], alg, w[0], w[1], (CfarOut)out, 0);
                                c.img_align = ia, c.out_align = oa, c.thr_align = out == CFAR_OUT_MASK_THR ? ta : 0;
                                if (out == CFAR_OUT_BITS && oa < 4) // the bit-stream entry point refuses it before the route
                                    continue;
                                checked_route(c, has_lut ? &lut : nullptr);
                            }
            g_what = "4096 frames of 2048 x 1024";
            for (int out = 0; out < 3; ++out)
                for (int variant = 0; variant < 4; ++variant)
                    checked_route(make(4096, 2048, 1024, alg, w[0], w[1], (CfarOut)out, variant), has_lut ? &lut : nullptr);
            g_what = "grid";
        }
}

// `(size_t)rows * cols < (1u << 30)` stood in the ring, slide and OS conditions
static void pixel_limit()
{
    g_what = "2^30 pixels";
    CfarLut lut;
    CHECK(build_lut(SFE_CFAR_SOCA, 20, 1.1, -1, &lut));
    struct {
        int rows, cols, alg;
        CfarOut out;
        CfarKernel want;
    } const cases[] = {
        {32768, 32764, SFE_CFAR_SOCA, CFAR_OUT_MASK, CFAR_RING},    // 2^30 - 131072 pixels
        {32768, 32768, SFE_CFAR_SOCA, CFAR_OUT_MASK, CFAR_GENERIC}, // 2^30
        {32768, 32736, SFE_CFAR_SOCA, CFAR_OUT_BITS, CFAR_RING},
        {32768, 32768, SFE_CFAR_SOCA, CFAR_OUT_BITS, CFAR_PACK},
        {4194304, 252, SFE_CFAR_SOCA, CFAR_OUT_MASK, CFAR_SLIDE_LDS}, // 2^30 - 2^24 pixels, cols < 256
        {4194304, 256, SFE_CFAR_SOCA, CFAR_OUT_MASK, CFAR_GENERIC},
        {32768, 32764, SFE_CFAR_OS, CFAR_OUT_MASK, CFAR_OS_PREF},
        {32768, 32768, SFE_CFAR_OS, CFAR_OUT_MASK, CFAR_GENERIC},
        {32768, 32764, SFE_CFAR_OS, CFAR_OUT_MASK_THR, CFAR_OS_HIST},
        {32768, 32768, SFE_CFAR_OS, CFAR_OUT_MASK_THR, CFAR_GENERIC},
    };
    for (const auto &k : cases) {
        const CfarRoute r = checked_route(make(1, k.rows, k.cols, k.alg, 20, 5, k.out, 0), &lut);
        CHECK(r.kernel == k.want);
    }
}

static void thr_arith()
{
    g_what = "cfar_thr_arith";
    const double taus[] = {9.137608674642355, 3.0, 0.1, 1.0 / 3.0, 7.123456789e5, 1e-300};
    const int trains[] = {40, 32, 20, 16, 24, 60};
    for (double tau : taus)
        for (int train : trains)
            for (int alg = SFE_CFAR_CA; alg <= SFE_CFAR_GOCA; ++alg) {
                g_c = make(1, 1, 1, alg, train / 2, 0, CFAR_OUT_MASK_THR, 0);
                g_c.tau = tau;
                CHECK(cfar_thr_arith_check(alg, train / 2, tau) == 1);
            }
}

static const char *const KERNEL_NAMES[] = {"none", "pack", "cfar_u8_ring", "cfar_u8_slide_lds", "cfar_u8_slide", "cfar_u8_os_gated",
                                           "cfar_u8_os_gated", "cfar_u8_os", "cfar_u8_generic"};

static std::string targs_of(const CfarCall &c, const CfarRoute &r)
{
    char b[64] = "";
    const char *const tf[] = {"false", "true"};
    if (r.kernel == CFAR_RING)
        std::snprintf(b, sizeof b, "%d,%d,%d,%d,%s,%s", c.T, c.G, c.alg, CFAR_RING_WINDOWS[r.instance].D,
                      tf[c.out == CFAR_OUT_BITS], tf[c.out == CFAR_OUT_MASK_THR]);
    else if (r.kernel == CFAR_SLIDE || r.kernel == CFAR_SLIDE_LDS)
        std::snprintf(b, sizeof b, "%d,%s", c.alg, tf[c.out == CFAR_OUT_MASK_THR]);
    else if (r.kernel == CFAR_OS_GATED || r.kernel == CFAR_OS_PREF)
        std::snprintf(b, sizeof b, "%s,%d", tf[r.v16], r.instance);
    return b;
}

// a line: name bits frames rows cols alg T G k tau gate thr img_align out_align thr_align variant tile_rows os_gated
// os_gated_min os_pref os_pref_x, then "refused" or: kernel targs|- workgroups wg_size packed
static int fixture(const char *path)
{
    g_what = "fixture";
    std::ifstream f(path);
    std::string line, name;
    int n = 0;
    while (std::getline(f, line)) {
        std::istringstream in(line);
        std::string kernel, targs;
        int bits, thr, packed = 0, wg_size = 0;
        long long workgroups = 0;
        CfarCall c;
        in >> name >> bits >> c.n_frames >> c.rows >> c.cols >> c.alg >> c.T >> c.G >> c.k >> c.tau >> c.intensity_thr >> thr >>
            c.img_align >> c.out_align >> c.thr_align >> c.variant >> c.tile_rows >> c.os_gated >> c.os_gated_min >> c.os_pref >>
            c.os_pref_x >> kernel;
        CHECK(!in.fail());
        g_what = name.c_str();
        c.out = bits ? CFAR_OUT_BITS : thr ? CFAR_OUT_MASK_THR : CFAR_OUT_MASK;
        c.thr_arith_on = thr && c.alg != SFE_CFAR_OS ? cfar_thr_arith_check(c.alg, c.T, c.tau) : 0;
        CfarLut lut;
        const bool has_lut = c.alg != SFE_CFAR_OS && build_lut(c.alg, c.T, c.tau, c.intensity_thr, &lut);
        CfarRoute r = checked_route(c, has_lut ? &lut : nullptr);
        if (kernel == "refused") {
            CHECK(r.ring_forced || r.refusal);
        } else {
            in >> targs >> workgroups >> wg_size >> packed;
            CHECK(!in.fail());
            CHECK(packed == (r.kernel == CFAR_PACK));
            if (packed) { // the byte kernels into the scratch mask (256-byte aligned), all frames at once
                c.out = CFAR_OUT_MASK, c.out_align = 16;
                r = checked_route(c, has_lut ? &lut : nullptr);
            }
            CHECK(r.kernel > CFAR_PACK && kernel == KERNEL_NAMES[r.kernel]);
            CHECK((targs == "-" ? "" : targs) == targs_of(c, r));
            CHECK(workgroups == r.workgroups && wg_size == (r.kernel == CFAR_OS_HIST ? 64 : 256));
        }
        ++n;
    }
    g_what = "fixture";
    CHECK(n > 0);
    return n;
}

int main(int argc, char **argv)
{
    invariants();
    pixel_limit();
    thr_arith();
    const int n = argc > 1 ? fixture(argv[1]) : 0;
    long long total = g_refused + g_forced;
    for (long long v : g_routes)
        total += v;
    std::printf("cfar_route_check: ok (%lld routes: %lld ring, %lld slide_lds, %lld slide, %lld os_gated, %lld os_pref, %lld os_hist, "
                "%lld generic, %lld pack, %lld ring forced; %d calls of the fixture)\n",
                total, g_routes[CFAR_RING], g_routes[CFAR_SLIDE_LDS], g_routes[CFAR_SLIDE], g_routes[CFAR_OS_GATED],
                g_routes[CFAR_OS_PREF], g_routes[CFAR_OS_HIST], g_routes[CFAR_GENERIC], g_routes[CFAR_PACK], g_forced, n);
    return 0;
}
