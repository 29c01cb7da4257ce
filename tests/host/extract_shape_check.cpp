// Stand-alone check of the launch-shape rules of extract_gather_kernel (sonar_slam_amd/csrc/sfe_extract_shape.h), run on
// the CPU: gather_shape() for every chunk size 1 .. 1024, with and without the record path, over frames of 1 word to
// 2^27 - 32 words (65535 rows of 65504 beams: the largest image the gather kernel takes), and the kernel's own index
// arithmetic from (slice, running word) to a word of the bit stream.  tests/test_extract_shape_rules.py builds it plainly;
// under the sanitizers it is a program of its own (no GPU, nothing preloaded):
//   g++ -std=c++17 -O1 -g -Wall -Wextra -Werror -fsanitize=address,undefined -fno-sanitize-recover=all
//       tests/host/extract_shape_check.cpp -o extract_shape_check && ./extract_shape_check
//
// What it asserts for every (nf, records, nwords):
//   * 1 <= slices <= 64, slices <= ceil(nwords / 64), slices + 2 <= 66 (s_rp of extract_merge_expand_kernel holds
//     s_rp[0 .. slices + 1]), 0 <= piece_shift <= 4;
//   * every slice owns at least one piece, and the slices' pieces add up to the frame's;
//   * over all slices and all running words v < my_words, the stream words gw < nwords are visited exactly once
//     (exhaustively up to 65536 words; beyond that by the first and last piece of every slice);
//   * no intermediate of the int arithmetic exceeds INT_MAX (everything is recomputed in 64 bits and compared);
//   * for frames 0, 1, 63, 64, 1023 of a launch, workgroup -> slice is a permutation of 0 .. slices - 1.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <tuple>
#include <vector>

#include "../../sonar_slam_amd/csrc/sfe_extract_shape.h"

static int g_nf = 0, g_records = 0;
static long long g_nwords = 0;
static GatherShape g_gs = {0, 0};

#define CHECK(cond)                                                                                                    \
    do {                                                                                                               \
        if (!(cond)) {                                                                                                 \
            std::fprintf(stderr, "extract_shape_check: %s fails (line %d): nf %d records %d nwords %lld -> slices %d " \
                                 "piece_shift %d\n",                                                                   \
                         #cond, __LINE__, g_nf, g_records, g_nwords, g_gs.slices, g_gs.piece_shift);                   \
            std::exit(1);                                                                                              \
        }                                                                                                              \
    } while (0)

// the kernel's arithmetic in 64 bits
struct Wide {
    long long pwords, npieces;
    Wide(long long nwords, int shift) : pwords(64ll << shift), npieces((nwords + (64ll << shift) - 1) >> (6 + shift)) {}
    long long my_pieces(int sl, int slices) const { return (npieces - sl + slices - 1) / slices; }
    long long word(int sl, long long v, int slices, int shift) const
    {
        return (sl + (v >> (6 + shift)) * slices) * pwords + (v & (pwords - 1));
    }
};

static long long g_words_walked = 0;

// the words a launch of `slices` workgroups looks at in one frame of nwords words
static void check_cover(int nwords, int slices, int shift, bool exhaustive)
{
    const Wide w(nwords, shift);
    CHECK(w.pwords <= INT_MAX && (long long)nwords + w.pwords - 1 <= INT_MAX);
    const int pwords = gather_piece_words(shift), npieces = gather_pieces(nwords, shift);
    CHECK(pwords == w.pwords && npieces == w.npieces);
    CHECK(npieces >= slices); // every slice owns at least one piece
    std::vector<unsigned char> seen(exhaustive ? (size_t)nwords : 0, 0);
    long long pieces = 0;
    for (int sl = 0; sl < slices; ++sl) {
        CHECK(w.npieces - sl + slices - 1 <= INT_MAX);
        const int my_pieces = gather_my_pieces(npieces, sl, slices);
        CHECK(my_pieces == w.my_pieces(sl, slices) && my_pieces >= 1);
        CHECK(w.my_pieces(sl, slices) * w.pwords <= INT_MAX);
        const int my_words = gather_my_words(my_pieces, shift);
        CHECK(my_words == w.my_pieces(sl, slices) * w.pwords);
        pieces += my_pieces;
        // the kernel evaluates gather_word for every v of a step of SG_BLOCK = 1024 words that begins below my_words, and
        // drops those beyond it: that must stay an int as well
        const long long v_end = (long long)my_words + 1024;
        CHECK(v_end <= INT_MAX && w.word(sl, v_end - 1, slices, shift) <= INT_MAX);
        // the first and the last piece of the slice: pieces sl and sl + (my_pieces - 1) * slices, whole
        const long long last_piece = sl + (long long)(my_pieces - 1) * slices;
        CHECK(last_piece < w.npieces && last_piece + slices >= w.npieces);
        CHECK(gather_word(sl, 0, slices, shift) == (long long)sl * w.pwords);
        CHECK(gather_word(sl, pwords - 1, slices, shift) == (long long)sl * w.pwords + w.pwords - 1);
        CHECK(gather_word(sl, my_words - pwords, slices, shift) == last_piece * w.pwords);
        CHECK(gather_word(sl, my_words - 1, slices, shift) == last_piece * w.pwords + w.pwords - 1);
        if (!exhaustive)
            continue;
        for (int v = 0; v < my_words; ++v) {
            const int gw = gather_word(sl, v, slices, shift);
            CHECK(gw == w.word(sl, v, slices, shift) && gw >= 0 && gw < w.npieces * w.pwords);
            if (gw < nwords) {
                CHECK(seen[(size_t)gw] == 0);
                seen[(size_t)gw] = 1;
            }
        }
        g_words_walked += my_words;
    }
    CHECK(pieces == w.npieces);
    for (size_t i = 0; i < seen.size(); ++i)
        CHECK(seen[i] == 1);
}

// `extract_shape_check --table NWORDS`: gather_shape for every chunk size, "records nf slices piece_shift" per line, for the
// Python copy of the slices rule (tools/extract_records_stats.py; compared by tests/test_extract_shape_rules.py)
static int table(long long nwords)
{
    for (int records = 0; records < 2; ++records)
        for (int nf = 1; nf <= 1024; ++nf) {
            const GatherShape gs = gather_shape(nwords, records != 0, nf);
            std::printf("%d %d %d %d\n", records, nf, gs.slices, gs.piece_shift);
        }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 3 && std::string(argv[1]) == "--table")
        return table(std::atoll(argv[2]));
    const long long sizes[] = {1, 2, 63, 64, 65, 100, 192, 1024, 4096, 4097, 16384, 65536, (1ll << 27) - 32};
    const unsigned frames[] = {0, 1, 63, 64, 1023};
    std::set<std::tuple<long long, int, int>> covered; // the cover depends on (nwords, slices, piece_shift) only
    long long combos = 0;
    for (long long nwords : sizes)
        for (int records = 0; records < 2; ++records)
            for (int nf = 1; nf <= 1024; ++nf) {
                g_nf = nf, g_records = records, g_nwords = nwords;
                const GatherShape gs = g_gs = gather_shape(nwords, records != 0, nf);
                CHECK(gs.slices >= 1 && gs.slices <= SFE_GATHER_MAX_SLICES && SFE_GATHER_MAX_SLICES == 64);
                CHECK(gs.slices <= (nwords + 63) / 64);
                CHECK(gs.slices + 2 <= 66);
                CHECK(gs.piece_shift >= 0 && gs.piece_shift <= 4);
                CHECK(nwords <= INT_MAX);
                if (covered.insert(std::make_tuple(nwords, gs.slices, gs.piece_shift)).second)
                    check_cover((int)nwords, gs.slices, gs.piece_shift, nwords <= 65536);
                for (unsigned f : frames) {
                    unsigned long long hit = 0;
                    for (unsigned bx = 0; bx < (unsigned)gs.slices; ++bx) {
                        const int sl = gather_slice_of(bx, f, gs.slices);
                        CHECK(sl >= 0 && sl < gs.slices && !((hit >> sl) & 1ull));
                        hit |= 1ull << sl;
                    }
                }
                ++combos;
            }
    std::printf("extract_shape_check: ok (%lld combinations, %zu distinct shapes, %lld words walked)\n", combos,
                covered.size(), g_words_walked);
    return 0;
}
