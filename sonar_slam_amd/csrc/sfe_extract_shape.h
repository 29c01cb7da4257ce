// Extraction, the launch shape of extract_gather_kernel: how many workgroups share a frame's bit stream (`slices`), the size
// of the pieces they take turns at (64 << piece_shift words), and which stream word a workgroup's running word index stands
// for.  Plain integer arithmetic without a HIP call, shared by the host (ExtractCall, sfe_extract.hip) and the kernel, so
// that the rules can be run on their own over every frame count (tests/host/extract_shape_check.cpp).
//
// `slices` also fixes the record layout that extract_merge_expand_kernel reads back: per frame `slices` regions of SG_TAB
// record slots + the spill region, `slices + 1` counters, and the merge kernel's s_rp[66] (64 regions + spill + total).
#pragma once

#if defined(__HIPCC__)
#define SFE_SHAPE_HD __host__ __device__
#else
#define SFE_SHAPE_HD
#endif

#define SFE_GATHER_MAX_SLICES 64

// Workgroups of the gather kernel per frame (`slices`, never more than 64: s_rp of the merge kernel holds 64 regions + the
// spill region) and the size of the pieces they take turns at, for a chunk of nf frames.
struct GatherShape {
    int slices, piece_shift;
};
// nwords: bit-stream words of a frame that hold pixels; records: the record path is on (ExtractRoute::records)
SFE_SHAPE_HD static inline GatherShape gather_shape(long long nwords, bool records, int nf)
{
    // workgroups per frame: enough of them to fill the device with a few frames, few enough that a
    // workgroup's list holds several rounds of 256 set pixels when there are many
    // 8192 workgroups per 512 frames measured best (16: 0.259 ms per 512 frames, 8: 0.274, 4: 0.36 -- a workgroup's
    // rounds of 256 set pixels wait for their loads one after the other), in pieces of 1024 words when the frame
    // has that many per workgroup (64 rows of 512 beams: a canvas word collects its bits from neighbouring rows,
    // so whole bands keep the table's words to one workgroup; 0.280 -> 0.259)
    // (record path: twice the workgroups per frame -- a workgroup's table of 1024 canvas words is its record region, and
    // at 8 workgroups per frame the densest bands of the bench's frames filled it: 77 spilled words per frame, each a
    // returning atomic, 2 % of the frames handed back; profiles/r05_extract_records_stats.txt.
    // Measured: 256 frames per launch 59.1 us with 32 workgroups per frame, 72.7 with 64; 512 frames 0.147 ms with 16, 0.165
    // with 32; 1024 frames 0.256 ms with 16.  So: 8192 workgroups per launch, but between 16 and 32 per frame for batches.)
    int slices = 8192 / (nf > 1 ? nf : 1);
    slices = slices > SFE_GATHER_MAX_SLICES ? SFE_GATHER_MAX_SLICES : slices < 2 ? 2 : slices;
    if (records && nf >= 64)
        slices = slices > 32 ? 32 : slices < 16 ? 16 : slices;
    const long long by_words = (nwords + 63) / 64; // a workgroup without a piece of its own would only idle
    if (slices > by_words)
        slices = (int)by_words;
    if (slices < 1)
        slices = 1;
    int piece = 4;
    while (piece > 0 && (nwords >> (6 + piece)) < slices)
        --piece;
    return {slices, piece};
}

// rotate the pieces from frame to frame: workgroups are dealt to the 8 XCDs in launch order, and every XCD should
// see every range band.  bx: the workgroup's index within its frame (blockIdx.x), f: the frame of the launch (blockIdx.y)
SFE_SHAPE_HD static inline int gather_slice_of(unsigned bx, unsigned f, int slices)
{
    return (int)((bx + 5u * f) % (unsigned)slices);
}

// pieces of 64 << piece_shift words (64 words = 4 polar rows of 512 beams); piece p belongs to slice p % slices
SFE_SHAPE_HD static inline int gather_piece_words(int piece_shift)
{
    return 64 << piece_shift;
}
SFE_SHAPE_HD static inline int gather_pieces(int nwords, int piece_shift)
{
    return (nwords + gather_piece_words(piece_shift) - 1) >> (6 + piece_shift);
}
SFE_SHAPE_HD static inline int gather_my_pieces(int npieces, int sl, int slices) // pieces sl, sl + slices, ...
{
    return (npieces - sl + slices - 1) / slices;
}
// the words of slice sl, piece after piece (the last piece of a frame may reach beyond nwords: the caller checks)
SFE_SHAPE_HD static inline int gather_my_words(int my_pieces, int piece_shift)
{
    return my_pieces * gather_piece_words(piece_shift);
}
// running word v of slice sl (0 <= v < gather_my_words) -> word of the frame's bit stream
SFE_SHAPE_HD static inline int gather_word(int sl, int v, int slices, int piece_shift)
{
    const int pwords = gather_piece_words(piece_shift);
    return (sl + (v >> (6 + piece_shift)) * slices) * pwords + (v & (pwords - 1));
}
