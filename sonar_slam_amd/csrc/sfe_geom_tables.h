// The host tables of a remap geometry (sfe_geom_create uploads them as they come out of here), each built by a plain
// function from plain arguments.  Nothing in this header calls HIP or knows sfe_geom, so a host-only program can include
// it and check the tables on their own.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#define SFE_CODE_NONE 0xFFFFFFFFu // remap code of a Cartesian pixel without a tap inside the polar image
#define EXTRACT_RG 32             // canvas rows per tile of the dense pass (extract_bits_kernel)

namespace sfe_tables {

struct alignas(8) Pair { // the layout of HIP's uint2
    uint32_t x, y;
};

// The packed remap code addresses (polar_rows + 1) x (polar_cols + 1) taps in 22 bits.
inline bool code_fits(int polar_rows, int polar_cols)
{
    return (long long)(polar_rows + 1) * (polar_cols + 1) <= (1ll << 22);
}

// rcp = ceil(2^32 / (polar_cols + 1)) for the in-kernel divide of the packed linear index; false when the multiply-high
// is not exact over the whole range of indices
inline bool exact_reciprocal(int polar_rows, int polar_cols, unsigned *rcp)
{
    const unsigned d = (unsigned)(polar_cols + 1);
    *rcp = (unsigned)((0x100000000ull + d - 1) / d);
    const unsigned lin_max = (unsigned)(polar_rows + 1) * d;
    for (unsigned lin = 0; lin < lin_max; ++lin)
        if ((unsigned)(((unsigned long long)lin * *rcp) >> 32) != lin / d)
            return false;
    return true;
}

inline int cv_round_f(float v)
{
    return (int)lrintf(v); // nearest-even in the default rounding mode == cvRound
}

// One uint32 per Cartesian pixel ([31:10] linear index of the top-left tap in the grid shifted by one, [9:0] = fy*32+fx;
// SFE_CODE_NONE = no tap inside the image) and per Cartesian row the [first, last) columns that have a code.
struct RemapCode {
    std::vector<uint32_t> code;
    std::vector<int32_t> span;
};
inline RemapCode remap_code(const float *map_x, const float *map_y, int cart_rows, int cart_cols, int polar_rows,
                            int polar_cols)
{
    RemapCode t;
    t.code.resize((size_t)cart_rows * cart_cols);
    t.span.resize(2 * (size_t)cart_rows);
    for (int r = 0; r < cart_rows; ++r) {
        int first = cart_cols, last = 0;
        for (int c = 0; c < cart_cols; ++c) {
            const size_t o = (size_t)r * cart_cols + c;
            const float mx = map_x[o] * 32.0f, my = map_y[o] * 32.0f;
            uint32_t cd = SFE_CODE_NONE;
            // |coordinate| < 2^20 px keeps cvRound and the >>5 well defined; anything larger is far outside
            if (std::fabs(mx) < 3.3e7f && std::fabs(my) < 3.3e7f) {
                const int sx = cv_round_f(mx), sy = cv_round_f(my);
                const int ix = sx >> 5, iy = sy >> 5;
                if (ix >= -1 && ix < polar_cols && iy >= -1 && iy < polar_rows) {
                    const uint32_t lin = (uint32_t)(iy + 1) * (uint32_t)(polar_cols + 1) + (uint32_t)(ix + 1);
                    cd = (lin << 10) | (uint32_t)((sy & 31) << 5) | (uint32_t)(sx & 31);
                    if (c < first)
                        first = c;
                    last = c + 1;
                }
            }
            t.code[o] = cd;
        }
        if (first > last)
            first = last = 0;
        t.span[2 * r] = first;
        t.span[2 * r + 1] = last;
    }
    return t;
}

// Per tile of the canvas (4 ballot words x EXTRACT_RG rows): the polar rows [ylo, yhi] its valid pixels tap, and the LDS
// the dense pass needs to stage the largest such range.
struct TileRows {
    int word_groups = 0, tiles_per_frame = 0;
    std::vector<int32_t> rows;
    int lds_bytes = 0;
};
inline TileRows tile_rows(const std::vector<uint32_t> &code, int cart_rows, int cart_cols, int polar_rows, int polar_cols)
{
    TileRows t;
    t.word_groups = ((cart_cols + 63) / 64 + 3) / 4;
    t.tiles_per_frame = t.word_groups * ((cart_rows + EXTRACT_RG - 1) / EXTRACT_RG);
    t.rows.resize(2 * (size_t)t.tiles_per_frame);
    long long max_words = 2;
    for (int tile = 0; tile < t.tiles_per_frame; ++tile) {
        const int wg = tile % t.word_groups, rg = tile / t.word_groups;
        int ylo = polar_rows, yhi = -1;
        for (int r = rg * EXTRACT_RG; r < std::min((rg + 1) * EXTRACT_RG, cart_rows); ++r)
            for (int c = wg * 256; c < std::min((wg + 1) * 256, cart_cols); ++c) {
                const uint32_t cd = code[(size_t)r * cart_cols + c];
                if (cd == SFE_CODE_NONE)
                    continue;
                const int iy = (int)((cd >> 10) / (uint32_t)(polar_cols + 1)) - 1;
                ylo = std::min(ylo, std::max(iy, 0));
                yhi = std::max(yhi, std::min(iy + 1, polar_rows - 1));
            }
        t.rows[2 * tile] = ylo;
        t.rows[2 * tile + 1] = yhi;
        if (ylo <= yhi)
            max_words = std::max(max_words, (long long)(yhi - ylo + 1) * ((polar_cols >> 5) | 1));
    }
    t.lds_bytes = (int)(max_words * 4);
    return t;
}

// The inverse map's entries carry the bit index of a canvas pixel inside a frame's bitmap in 32 bits.
inline bool bit_index_fits(int cart_rows, int words_per_row)
{
    return (unsigned long long)cart_rows * words_per_row * 64ull < (1ull << 32) - 1;
}

// Inverse map: polar pixel -> the canvas pixels that tap it with a non-zero weight (same weights as the kernels), CSR:
// off[polar_rows * polar_cols + 1], entry = {bit index of the canvas pixel inside a frame's bitmap (row * words_per_row * 64
// + col: the gather kernel sets that bit without dividing by the canvas width), its remap code}, sorted by canvas pixel.
struct InverseMap {
    std::vector<int32_t> off;
    std::vector<Pair> ent;
};
inline InverseMap inverse_map(const std::vector<uint32_t> &code, int cart_cols, int polar_rows, int polar_cols,
                              int words_per_row)
{
    InverseMap m;
    m.off.assign((size_t)polar_rows * polar_cols + 1, 0);
    const size_t n = code.size();
    auto each_tap = [&](size_t o, auto &&fn) {
        const uint32_t cd = code[o];
        if (cd == SFE_CODE_NONE)
            return;
        const uint32_t lin = cd >> 10;
        const int fy = (int)((cd >> 5) & 31u), fx = (int)(cd & 31u);
        const int iy = (int)(lin / (uint32_t)(polar_cols + 1)) - 1, ix = (int)(lin % (uint32_t)(polar_cols + 1)) - 1;
        int wgt[4] = {(32 - fy) * (32 - fx), (32 - fy) * fx, fy * (32 - fx), fy * fx};
        if ((fx | fy) == 0)
            wgt[3] = 1;
        for (int t = 0; t < 4; ++t) {
            const int y = iy + (t >> 1), x = ix + (t & 1);
            if (wgt[t] > 0 && y >= 0 && y < polar_rows && x >= 0 && x < polar_cols)
                fn((size_t)y * polar_cols + x);
        }
    };
    for (size_t o = 0; o < n; ++o)
        each_tap(o, [&](size_t pi) { ++m.off[pi + 1]; });
    for (size_t i = 1; i < m.off.size(); ++i)
        m.off[i] += m.off[i - 1];
    m.ent.resize((size_t)m.off.back());
    std::vector<int32_t> cur(m.off.begin(), m.off.end() - 1);
    for (size_t o = 0; o < n; ++o)
        each_tap(o, [&](size_t pi) {
            const size_t row = o / (size_t)cart_cols, col = o - row * (size_t)cart_cols;
            m.ent[(size_t)cur[pi]++] = Pair{(uint32_t)(row * (size_t)words_per_row * 64 + col), code[o]};
        });
    return m;
}

// The same entries with the blend decided in advance (extract_gather_kernel).  Whether a canvas pixel reached from one of
// its set taps is a detection -- and whether THIS tap is the one that reports it -- depends on the entry (the tap's place
// among the four, the two 5-bit fractions) and on the four mask bits of the taps only: 16 cases, evaluated here with the
// kernels' arithmetic.  y = table (bit p: taps v00 v01 v10 v11 = bits 0..3 of p) | shift << 16, shift = position of tap 00
// inside the 3 x 3 neighbourhood of the set pixel (bit 3 * (dy + 1) + dx + 1).  Two empty entries follow the last one: the
// kernel reads entries in pairs.
inline std::vector<Pair> blend_table(const InverseMap &m, int polar_cols)
{
    std::vector<Pair> lut(m.ent.size() + 2, Pair{0u, 0u});
    for (size_t pi = 0; pi + 1 < m.off.size(); ++pi) {
        const int py = (int)(pi / (size_t)polar_cols), px = (int)(pi - (size_t)py * polar_cols);
        for (int32_t j = m.off[pi]; j < m.off[pi + 1]; ++j) {
            const uint32_t cd = m.ent[(size_t)j].y, lin = cd >> 10;
            const int fy = (int)((cd >> 5) & 31u), fx = (int)(cd & 31u);
            const int iy = (int)(lin / (uint32_t)(polar_cols + 1)) - 1, ix = (int)(lin % (uint32_t)(polar_cols + 1)) - 1;
            const int ry = iy - py + 1, rx = ix - px + 1; // 0 or 1
            int w00 = (32 - fy) * (32 - fx) * 32, w01 = (32 - fy) * fx * 32, w10 = fy * (32 - fx) * 32, w11 = fy * fx * 32;
            if ((fx | fy) == 0) {
                w00 = 32767;
                w11 = 1;
            }
            const int t_src = (1 - ry) * 2 + (1 - rx);
            uint32_t tab = 0;
            for (int p = 0; p < 16; ++p) {
                const int v00 = p & 1, v01 = (p >> 1) & 1, v10 = (p >> 2) & 1, v11 = (p >> 3) & 1;
                const int acc = w00 * v00 + w01 * v01 + w10 * v10 + w11 * v11;
                const int first = (v00 && w00) ? 0 : (v01 && w01) ? 1 : (v10 && w10) ? 2 : 3;
                if (((acc + 16384) >> 15) != 0 && t_src == first)
                    tab |= 1u << p;
            }
            lut[(size_t)j] = Pair{m.ent[(size_t)j].x, tab | ((uint32_t)(ry * 3 + rx) << 16)};
        }
    }
    return lut;
}

// The blend table in 4 bytes per entry {table [15:0], tap place [17:16], dx [24:18], dy [31:25]}, relative to a base bit
// index per polar pixel (ob: {offset into c4, base}), without the entries whose table is 0 (extract_gather_kernel<true>).
// fits = false when a pixel's candidates span more than 127 canvas rows / columns (no sonar fan does): the 8-byte entries
// are then all there is.  Eight empty entries follow the last one (the kernel reads entries in fours, two reads ahead) and
// one more {offset, base} pair closes ob (16-byte reads of pairs).
struct CompactMap {
    bool fits = true;
    std::vector<Pair> ob;
    std::vector<uint32_t> c4;
};
inline CompactMap compact_map(const std::vector<int32_t> &off, const std::vector<Pair> &lut, int words_per_row)
{
    CompactMap m;
    const size_t npix = off.size() - 1;
    m.ob.resize(npix + 1);
    m.c4.reserve((size_t)off.back());
    const unsigned long long rowbits = (unsigned long long)words_per_row * 64ull;
    for (size_t pi = 0; pi < npix && m.fits; ++pi) {
        unsigned long long rmin = ~0ull, cmin = ~0ull;
        for (int32_t j = off[pi]; j < off[pi + 1]; ++j)
            if (lut[(size_t)j].y & 0xFFFFu) {
                rmin = std::min<unsigned long long>(rmin, lut[(size_t)j].x / rowbits);
                cmin = std::min<unsigned long long>(cmin, lut[(size_t)j].x % rowbits);
            }
        if (rmin == ~0ull)
            rmin = cmin = 0;
        m.ob[pi] = Pair{(uint32_t)m.c4.size(), (uint32_t)(rmin * rowbits + cmin)};
        for (int32_t j = off[pi]; j < off[pi + 1]; ++j) {
            const Pair e = lut[(size_t)j];
            if (!(e.y & 0xFFFFu))
                continue;
            const unsigned long long dy = e.x / rowbits - rmin, dx = e.x % rowbits - cmin;
            const unsigned shift = e.y >> 16, sc = shift >= 3 ? shift - 1 : shift; // ry * 3 + rx -> ry * 2 + rx
            if (dy > 127 || dx > 127 || m.c4.size() >= 0xFFFFFFF0ull) {
                m.fits = false;
                break;
            }
            m.c4.push_back((e.y & 0xFFFFu) | (sc << 16) | ((uint32_t)dx << 18) | ((uint32_t)dy << 25));
        }
    }
    if (!m.fits)
        return m;
    m.ob[npix] = Pair{(uint32_t)m.c4.size(), 0u};
    m.c4.resize(m.c4.size() + 8, 0u);
    m.ob.resize(m.ob.size() + 1, Pair{(uint32_t)m.c4.size(), 0u});
    return m;
}

// px -> m per canvas row / column: the fp64 expressions of feature_extraction.py:236-237 in the reference's operation order
struct MetreTables {
    std::vector<double> ytab, xtab;
};
inline MetreTables metre_tables(int cart_rows, int cart_cols, double width, double height)
{
    MetreTables t;
    t.ytab.resize((size_t)cart_rows);
    t.xtab.resize((size_t)cart_cols);
    const double half_cols = cart_cols / 2.;
    for (int r = 0; r < cart_rows; ++r)
        t.ytab[(size_t)r] = (-1 * ((double)r / (double)cart_rows) * height) + height; // feature_extraction.py:237
    for (int c = 0; c < cart_cols; ++c) {
        double x = (double)c - half_cols;                                              // feature_extraction.py:236
        t.xtab[(size_t)c] = (-1 * ((x / half_cols) * (width / 2.)));
    }
    return t;
}

} // namespace sfe_tables
