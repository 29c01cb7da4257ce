// sfe_geom: what the remap and extraction kernels know about one polar -> Cartesian geometry.  The float maps are decoded
// ONCE per geometry (layout of the packed remap code: sfe_remap.hip); every table is built on the host by a plain function
// of sfe_geom_tables.h and uploaded here.
#include "sfe_internal.h"
#include "sfe_geom_tables.h"

namespace {

// allocate, copy, record the pointer; after a failure nothing more is tried and `failed` names the table
struct GeomUpload {
    const char *failed = nullptr;
    template <typename D, typename T> void operator()(D *&dst, const std::vector<T> &v, const char *name)
    {
        static_assert(sizeof(D) == sizeof(T), "the host table has the device table's element size");
        if (failed)
            return;
        const size_t bytes = v.size() * sizeof(T);
        if (hipMalloc((void **)&dst, std::max<size_t>(bytes, 1)) != hipSuccess ||
            (bytes && hipMemcpy(dst, v.data(), bytes, hipMemcpyHostToDevice) != hipSuccess))
            failed = name;
    }
};

} // namespace

extern "C" {

int sfe_geom_create(sfe_ctx *ctx, const float *map_x, const float *map_y, int cart_rows, int cart_cols,
                    int polar_rows, int polar_cols, double width, double height, sfe_geom **out)
{
    using namespace sfe_tables;
    if (int rc = sfe_use(ctx))
        return rc;
    SFE_ARG(ctx, out && map_x && map_y);
    *out = nullptr;
    SFE_ARG(ctx, cart_rows > 0 && cart_cols > 0 && polar_rows > 0 && polar_cols > 0);
    if (!code_fits(polar_rows, polar_cols))
        return sfe_set_err(ctx, SFE_ERR_ARG, "polar image %dx%d too large for the packed remap code (max 2^22 px)",
                           polar_rows, polar_cols);
    unsigned rcp = 0;
    if (!exact_reciprocal(polar_rows, polar_cols, &rcp))
        return sfe_set_err(ctx, SFE_ERR_ARG, "reciprocal divide not exact for polar_cols=%d", polar_cols);

    const int words_per_row = (cart_cols + 63) / 64;
    const RemapCode codes = remap_code(map_x, map_y, cart_rows, cart_cols, polar_rows, polar_cols);
    const TileRows tiles = tile_rows(codes.code, cart_rows, cart_cols, polar_rows, polar_cols);
    if (tiles.lds_bytes > 150 * 1024)
        return sfe_set_err(ctx, SFE_ERR_ARG, "geometry needs %d bytes of LDS per canvas tile (max 153600)", tiles.lds_bytes);
    // the inverse map's offsets are 32-bit: a canvas of 2^32 pixels or more goes without (dense pass only)
    const bool inverse = codes.code.size() < (1ull << 32);
    if (inverse && !bit_index_fits(cart_rows, words_per_row))
        return sfe_set_err(ctx, SFE_ERR_ARG, "canvas %dx%d too large for the inverse map's 32-bit bit index", cart_rows, cart_cols);
    InverseMap inv;
    std::vector<Pair> lut;
    CompactMap compact;
    compact.fits = false;
    if (inverse) {
        inv = inverse_map(codes.code, cart_cols, polar_rows, polar_cols, words_per_row);
        lut = blend_table(inv, polar_cols);
        compact = compact_map(inv.off, lut, words_per_row);
    }
    const MetreTables metres = metre_tables(cart_rows, cart_cols, width, height);

    sfe_geom *g = new sfe_geom();
    g->ctx = ctx;
    g->cart_rows = cart_rows;
    g->cart_cols = cart_cols;
    g->polar_rows = polar_rows;
    g->polar_cols = polar_cols;
    g->width = width;
    g->height = height;
    g->words_per_row = words_per_row;
    g->rcp = rcp;
    g->word_groups = tiles.word_groups;
    g->tiles_per_frame = tiles.tiles_per_frame;
    g->lds_bytes = tiles.lds_bytes;
    GeomUpload up;
    if (compact.fits) {
        up(g->d_inv_ob, compact.ob, "compact inverse map offsets");
        up(g->d_inv_c4, compact.c4, "compact inverse map entries");
    }
    if (inverse) {
        // (the {canvas pixel, remap code} entries themselves stay on the host: only their blend tables are read)
        up(g->d_inv_lut, lut, "inverse map entries");
        up(g->d_inv_off, inv.off, "inverse map offsets");
    }
    up(g->d_ytab, metres.ytab, "px->m rows");
    up(g->d_xtab, metres.xtab, "px->m columns");
    up(g->d_code, codes.code, "remap code");
    up(g->d_span, codes.span, "row spans");
    up(g->d_tile_rows, tiles.rows, "tile rows");
    if (up.failed) {
        sfe_geom_destroy(g);
        return sfe_set_err(ctx, SFE_ERR_HIP, "geometry upload failed: %s table", up.failed);
    }
    *out = g;
    return 0;
}

void sfe_geom_destroy(sfe_geom *g)
{
    if (!g)
        return;
    if (g->ctx) {
        (void)hipSetDevice(g->ctx->device);
        (void)hipStreamSynchronize(g->ctx->stream);
    }
    void *const tables[] = {g->d_code,   g->d_span,   g->d_tile_rows, g->d_inv_off, g->d_inv_lut,
                            g->d_inv_ob, g->d_inv_c4, g->d_ytab,      g->d_xtab};
    for (void *p : tables)
        if (p)
            (void)hipFree(p);
    delete g;
}

} // extern "C"
