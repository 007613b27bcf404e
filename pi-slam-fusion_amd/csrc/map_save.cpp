// map_save.cpp -- the whole mosaic (fusion_map.hpp): save_mosaic and its targets -- memory, files, web tiles.
#include "fusion_map.hpp"
#include "map_internal.hpp"
#include "env.hpp"
#include "coverage.hpp"
#include "webtiles_plan.hpp"
#include <algorithm>
#include <cstdio>
#include <cstring>

namespace pf {

// ------------------------------------------------------------------- save
// MultiBandMap2DCPU::save (.cpp:779-847): paste all tiles per level, collapse
// the whole mosaic once, 8U, background where level-0 weight is 0.  Everything between the extent and the hand-over of the
// pixels happens under one hold of mu_: the buffer a target is given and the mosaic written into it have the same extent.
bool FusionMap::save_mosaic(SaveTarget& t, const std::vector<ForeignTile>* foreign)
{
    Drained l(*this);
    if (!init_ok_ || !valid_ || !set_device()) return false;
    if (w_ == 0 || h_ == 0) return false;
    Section sec(this, T_SAVE);
    int mnx = 1000000, mny = 1000000, mxx = -1000000, mxy = -1000000, cnt = 0;
    store_.for_each([&](int ix, int iy, Tile& tile) {
        if (tile.fresh) return;
        cnt++; mnx = std::min(mnx, ix); mny = std::min(mny, iy); mxx = std::max(mxx, ix); mxy = std::max(mxy, iy);
    });
    if (foreign) for (auto& f : *foreign) { cnt++; mnx = std::min(mnx, f.ix); mny = std::min(mny, f.iy); mxx = std::max(mxx, f.ix); mxy = std::max(mxy, f.iy); }
    if (!cnt) return false;
    t.found = true;
    const int wx = mxx + 1 - mnx, wy = mxy + 1 - mny;
    const int level = t.level;                      // 0 but for pf_save_to_memory_level (checked there: Extent / Buffer without mask)
    t.rows = wy * (kElePixels >> level); t.cols = wx * (kElePixels >> level); t.tx0 = mnx; t.ty0 = mny;
    for (double& v : t.transform) v = 0;
    t.transform[0] = length_pixel_ * (1 << level); t.transform[3] = min_[0] + (mnx - off_x_) * ele_size_;
    t.transform[5] = length_pixel_ * (1 << level); t.transform[7] = min_[1] + (mny - off_y_) * ele_size_;
    t.transform[10] = 1; t.transform[15] = 1;
    std::memcpy(t.plane7, plane_.t, 24); std::memcpy(t.plane7 + 3, plane_.q, 32);
    if (t.kind == SaveTarget::Extent) return true;
    const bool file = t.kind == SaveTarget::File, web = t.kind == SaveTarget::Tiles;
    if (web && (single_band_ || !t.web)) { set_error("save: map tiles of a mosaic in HBM were asked for where there is none"); return false; }
    if (file && single_band_) { set_error("save: the stream of a mosaic in HBM was asked for where there is none"); return false; }
    if (file && t.route == SaveRoute::DeviceJpeg && !jpeg_size_ok("save", t.rows, t.cols)) return false;          // before anything is made: no file
    const size_t out_bytes = (size_t)t.rows * t.cols * 3, mask_bytes = (size_t)t.rows * t.cols;
    if (t.kind == SaveTarget::Image) { t.image->resize(out_bytes); if (t.mask_image) t.mask_image->resize(mask_bytes); }
    uint8_t* const bgr = file ? nullptr : t.kind == SaveTarget::Image ? t.image->data() : t.bgr;
    uint8_t* const mask = file ? nullptr : t.kind == SaveTarget::Image ? (t.mask_image ? t.mask_image->data() : nullptr) : t.mask;
    if (single_band_) {          // Map2DCPU::save (Map2DCPU.cpp:523-563): paste the tiles; holes are zero here
        HIP_OK(sync_all());
        if (bgr) std::memset(bgr, 0, out_bytes);
        if (mask) std::memset(mask, 0, mask_bytes);          // covered: the tile's alpha byte, the winning weight, is not 0
        std::vector<uint8_t> px((size_t)kElePixels * kElePixels * 4);
        bool ok = true;
        store_.for_each([&](int ix, int iy, Tile& tile) {
            if (tile.fresh || !ok) return;
            if (hipMemcpy(px.data(), tile.base, px.size(), hipMemcpyDeviceToHost) != hipSuccess) { ok = false; return; }
            for (int r = 0; r < kElePixels; r++) {
                const size_t o = ((size_t)(iy - mny) * kElePixels + r) * t.cols + (size_t)(ix - mnx) * kElePixels;
                if (bgr) bgra_to_bgr(px.data() + (size_t)r * kElePixels * 4, bgr + o * 3, kElePixels);
                if (mask) for (int x = 0; x < kElePixels; x++) mask[o + x] = px[((size_t)r * kElePixels + x) * 4 + 3] ? 255 : 0;
            }
        });
        return ok;
    }
    const int L = band_num_;
    const size_t es = lay_.f32 ? 4 : 2, px = 3 * es;
    std::vector<uint64_t> tab((size_t)wx * wy, 0);
    store_.for_each([&](int ix, int iy, Tile& tile) { if (!tile.fresh) tab[(size_t)(iy - mny) * wx + (ix - mnx)] = (uint64_t)(uintptr_t)tile.base; });
    if (foreign) for (auto& f : *foreign) tab[(size_t)(f.iy - mny) * wx + (f.ix - mnx)] = (uint64_t)(uintptr_t)f.dev;
    HIP_OK(sync_all());
    if (!mosaic_table_.reserve(tab.size() * 8)) return false;
    HIP_OK(hipMemcpy(mosaic_table_.p, tab.data(), tab.size() * 8, hipMemcpyHostToDevice));
    if (!blend_out_bgr_.reserve(out_bytes)) return false;
#if PF_EXPERIMENTS
    static const bool per_level = exp_env("PF_BLEND_PER_LEVEL") != nullptr;
    if (per_level && bgr && !mask && level == 0) {                // rounds 1-5: paste per level, one collapse launch per level, finish
        for (int i = 0; i <= L; i++) {
            const size_t n = (size_t)(t.rows >> i) * (t.cols >> i);
            if (!blend_lv_[i].reserve(n * px)) return false;
            prof_begin(K_MOSAIC_GATHER, (double)n * px * 2);
            launch_mosaic_gather(stream_, lay_, i, (const uint64_t*)mosaic_table_.p, wx, wy, blend_lv_[i].p);
            prof_end();
        }
        for (int i = L; i > 0; i--) {
            prof_begin(K_COLLAPSE, (double)(t.rows >> (i - 1)) * (t.cols >> (i - 1)) * px * 2.25);
            launch_collapse(stream_, lay_.f32, blend_lv_[i - 1].p, 0, blend_lv_[i].p, 0, t.rows >> (i - 1), t.cols >> (i - 1), 1);
            prof_end();
        }
        prof_begin(K_SAVE_FINISH, (double)t.rows * t.cols * (px + 4 + 3));
        launch_save_finish(stream_, lay_, blend_lv_[0].p, (const uint64_t*)mosaic_table_.p, wx, wy, opt_.bg_color, (uint8_t*)blend_out_bgr_.p);
        prof_end();
        HIP_OK(sync_all());
        HIP_OK(hipMemcpy(bgr, blend_out_bgr_.p, out_bytes, hipMemcpyDeviceToHost));
        return true;
    }
#endif
    // one launch: paste, collapse in LDS from level `level` down, 8U, background (level 0: collapse_fused.hip, above: collapse_level.hip).
    // Algorithmic bytes: every tile's Laplacians of levels level .. L and that level's weights read once, the mosaic written once.
    // A request for the mask alone (Buffer without bgr) needs no pixels
    if (file || bgr || web) {
        double P = 0; for (int i = level; i <= L; i++) P += 1.0 / (double)(1 << (2 * i));
        prof_begin(level ? K_SAVE_LEVEL : K_SAVE_FUSED, (double)cnt * kElePixels * kElePixels * (P * px + 4.0 / (double)(1 << (2 * level))) + (double)out_bytes);
        if (level) launch_save_level(stream_, lay_, level, (const uint64_t*)mosaic_table_.p, wx, wy, opt_.bg_color, (uint8_t*)blend_out_bgr_.p);
        else launch_save_fused(stream_, lay_, (const uint64_t*)mosaic_table_.p, wx, wy, opt_.bg_color, (uint8_t*)blend_out_bgr_.p);
        prof_end();
        HIP_OK(hipGetLastError());
    }
    // the coverage from the same table, in cover_bytes_: the level-0 weights' "!= 0" bits (coverage.hip), spread to bytes
    auto coverage = [&]() -> bool {
        if (!cover_plane_.reserve(mask_bytes / 8) || !cover_bytes_.reserve(mask_bytes)) return false;
        launch_coverage_tiles(stream_, (const uint64_t*)mosaic_table_.p, wx, wy, lay_.w_off[0], (uint8_t*)cover_plane_.p, nullptr, nullptr);
        launch_coverage_expand(stream_, (const uint8_t*)cover_plane_.p, t.rows, t.cols, (uint8_t*)cover_bytes_.p);
        HIP_OK(hipGetLastError());
        return true;
    };
    if (web) return coverage() && export_webtiles(t, *t.web);          // sampled from the mosaic and the coverage where both lie; streams, masks and flags cross to the host
    if (!file) {
        std::vector<OutPiece> pieces;
        if (bgr) pieces.push_back({ bgr, blend_out_bgr_.p, out_bytes });
        if (mask) {
            if (!coverage()) return false;
            pieces.push_back({ mask, cover_bytes_.p, mask_bytes });
        }
        return out_ring_.download(stream_, pieces);
    }
    // the mosaic stays where the collapse left it
    if (t.route == SaveRoute::DeviceTiff || t.route == SaveRoute::DeviceTiffLossless) {        // overviews, empty test and tile streams are made from it there; the masks from the table
        TiffDevice::Mask mk;
        mk.dev_table = (const uint64_t*)mosaic_table_.p; mk.wx = wx; mk.wy = wy; mk.w_off = lay_.w_off[0];
        return tiff_dev_.write(t.name, blend_out_bgr_.p, t.rows, t.cols, (size_t)t.cols * 3, t.quality, opt_.bg_color, t.transform, t.force_bigtiff, jpeg_enc_, stream_,
                               t.masked ? &mk : nullptr, t.route == SaveRoute::DeviceTiffLossless ? &deflate_enc_ : nullptr);
    }
    if (t.route == SaveRoute::DevicePng) {          // the whole file is made in HBM and crosses once
        if (t.masked && !coverage()) return false;
        size_t step = 0, mask_step = 0, len = 0;
        if (!png_args_ok("save_png", blend_out_bgr_.p, t.rows, t.cols, step, t.masked ? cover_bytes_.p : nullptr, mask_step)) return false;          // before anything is made: no file
        if (!png_enc_.encode(blend_out_bgr_.p, t.rows, t.cols, step, t.masked ? cover_bytes_.p : nullptr, mask_step, &len, stream_)) return false;
        const uint8_t* file_bytes = png_enc_.fetch_pinned(stream_);
        if (!file_bytes) return false;
        if (!write_bytes_file(t.name, file_bytes, len)) { std::remove(t.name); return false; }
        return true;
    }
    size_t off[2];                                 // cv::imwrite's JPEG defaults: quality 95, 4:2:0
    if (!jpeg_enc_.encode(blend_out_bgr_.p, 1, nullptr, 0, t.rows, t.cols, (size_t)t.cols * 3, t.quality, off, stream_)) return false;
    const uint8_t* stream = jpeg_enc_.fetch_pinned(stream_);
    return stream && write_bytes_file(t.name, stream, off[1]);
}

// the mosaic of extent t in blend_out_bgr_ and its coverage in cover_bytes_ as the map tiles of `job`: where the mosaic lies on the
// globe (reported to the caller who asked), then sampled, reduced and encoded on the GPU (webtiles.hip)
bool FusionMap::export_webtiles(const SaveTarget& t, const WebTilesJob& job)
{
    double px2ll[6];
    webtiles::georef_compose(t.transform, t.plane7, job.gps_origin, px2ll);
    if (job.report) { std::memcpy(job.report, px2ll, sizeof px2ll); job.report[6] = t.rows; job.report[7] = t.cols; }
    return webtiles_export(blend_out_bgr_.p, t.rows, t.cols, (size_t)t.cols * 3, cover_bytes_.p, (size_t)t.cols, px2ll, job.zmin, job.zmax, job.quality, opt_.bg_color,
                           job.want_pixels, job.sink, job.user, jpeg_enc_, stream_);
}

// the two-call protocols' end: save_mosaic(), then the extent handed back
bool FusionMap::save_to_caller(SaveTarget& t, int* rows, int* cols, int* tx0, int* ty0)
{
    if (!save_mosaic(t)) return false;
    *rows = t.rows; *cols = t.cols; *tx0 = t.tx0; *ty0 = t.ty0;
    return true;
}

bool FusionMap::save_to_memory_mask(uint8_t* bgr, uint8_t* mask, int* rows, int* cols, int* tx0, int* ty0)
{
    SaveTarget t;
    t.kind = bgr || mask ? SaveTarget::Buffer : SaveTarget::Extent; t.bgr = bgr; t.mask = mask;
    return save_to_caller(t, rows, cols, tx0, ty0);
}

// the two-call protocol of pf_save_to_memory at pyramid level `level`: the extent is wy E x wx E, E = 256 >> level
bool FusionMap::save_to_memory_level(int level, uint8_t* bgr, int* rows, int* cols, int* tx0, int* ty0)
{
    if (!level_ok("pf_save_to_memory_level", level)) return false;
    SaveTarget t;
    t.kind = bgr ? SaveTarget::Buffer : SaveTarget::Extent; t.bgr = bgr; t.level = level;
    return save_to_caller(t, rows, cols, tx0, ty0);
}

bool FusionMap::webtiles_georef(const double gps_origin[3], double px2ll[6], int* rows, int* cols)
{
    if (opt_.shard_count > 1) { set_error("pf_webtiles: a sharded map (shard_count > 1) holds a part of the mosaic only: gather it (pf_dist_save_to_memory) and use pf_webtiles_device"); return false; }
    SaveTarget t;
    if (!save_mosaic(t)) { set_error("pf_webtiles: the map has no content"); return false; }
    double p[6], A[4];
    webtiles::georef_compose(t.transform, t.plane7, gps_origin, p);
    if (!webtiles::invert2(p, A)) { set_error(std::string("pf_webtiles: ") + webtiles::plan_message(webtiles::kPlanSingular)); return false; }
    std::memcpy(px2ll, p, sizeof p);
    if (rows) *rows = t.rows;
    if (cols) *cols = t.cols;
    return true;
}

bool FusionMap::webtiles(const WebTilesJob& job)
{
    if (opt_.shard_count > 1) { set_error("pf_webtiles: a sharded map (shard_count > 1) holds a part of the mosaic only: gather it (pf_dist_save_to_memory) and use pf_webtiles_device"); return false; }
    SaveTarget t;
    if (!single_band_) {
        t.kind = SaveTarget::Tiles; t.web = &job;
        if (save_mosaic(t)) return true;
        if (!t.found) set_error("pf_webtiles: the map has no content");
        return false;
    }
    // Map2DCPU semantics: the host mosaic and its alpha mask of one moment, uploaded, through the same device path
    std::vector<uint8_t> img, cover;
    t.kind = SaveTarget::Image; t.image = &img; t.mask_image = &cover;
    if (!save_mosaic(t)) { set_error("pf_webtiles: the map has no content"); return false; }
    std::lock_guard<std::mutex> l(mu_);
    if (!set_device()) return false;
    if (!blend_out_bgr_.reserve(img.size()) || !cover_bytes_.reserve(cover.size())) return false;
    HIP_OK(hipMemcpy(blend_out_bgr_.p, img.data(), img.size(), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(cover_bytes_.p, cover.data(), cover.size(), hipMemcpyHostToDevice));
    return export_webtiles(t, job);
}

bool FusionMap::save_file(const char* filename, SaveRoute route, int quality, bool force_bigtiff, const std::vector<ForeignTile>* foreign, bool masked)
{
    std::vector<uint8_t> img, cover;
    SaveTarget t;
    if (route_on_device(route)) { t.kind = SaveTarget::File; t.name = filename; t.route = route; t.quality = quality; t.force_bigtiff = force_bigtiff; t.masked = masked; }
    else { t.kind = SaveTarget::Image; t.image = &img; if (masked) t.mask_image = &cover; }
    if (!save_mosaic(t, foreign)) return false;
    if (route == SaveRoute::HostTiffGeo) {
        if (masked ? !write_tiff_masked_file("save", filename, img.data(), t.rows, t.cols, 0, cover.data(), 0, quality, opt_.bg_color, t.transform, force_bigtiff)
                   : !write_tiff_file("save", filename, img.data(), t.rows, t.cols, 0, quality, opt_.bg_color, t.transform, force_bigtiff)) return false;
    }
    if (route == SaveRoute::HostTiffLossless &&
        !write_tiff_lossless_file("save", filename, img.data(), t.rows, t.cols, 0, masked ? cover.data() : nullptr, 0, opt_.bg_color, t.transform, force_bigtiff)) return false;
    if (route == SaveRoute::HostPng && !write_png_file("save_png", filename, img.data(), t.rows, t.cols, 0, masked ? cover.data() : nullptr, 0)) return false;
    if (route == SaveRoute::HostImage && !write_image_file(filename, img.data(), t.rows, t.cols)) return false;
    std::printf("Resolution:[%d %d]\n", t.cols, t.rows);
    return true;
}

}  // namespace pf
