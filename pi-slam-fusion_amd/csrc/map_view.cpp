// map_view.cpp -- views of the mosaic (fusion_map.hpp, DESIGN.md "Views"): the plan (view_plan.hpp), the collapse of the tiles the view
// depends on, their coverage, the warp (view.hip) and the three ways out -- host memory, a caller's device memory, a JPEG stream.
#include "fusion_map.hpp"
#include "map_internal.hpp"
#include "view.hpp"
#include "view_plan.hpp"
#include <algorithm>
#include <cstring>

namespace pf {

bool FusionMap::render_view(const double V[9], int width, int height, int level, const ViewTarget& t, pf_view_info* info_out)
{
    const char* who = t.kind == ViewTarget::Jpeg ? "pf_render_view_jpeg" : t.kind == ViewTarget::Device ? "pf_render_view_device" : "pf_render_view";
    auto refuse = [&](const std::string& why) { set_error(std::string(who) + ": " + why); return false; };
    if (single_band_) return refuse("a TypeCPU / TypeGPU map holds no pyramid to take a view from");
    if (opt_.shard_count > 1) return refuse("a sharded map (shard_count > 1) holds a part of the mosaic only: gather it (pf_dist_save_to_memory)");
    const int channels = t.kind == ViewTarget::Jpeg ? 3 : t.channels;
    if (channels != 3 && channels != 4) return refuse("3 or 4 channels");
    Drained l(*this);
    if (!init_ok_ || !valid_) return refuse("the map is not prepared");
    if (!set_device()) return false;
    // the content's extent, as save() takes it
    int mnx = 1000000, mny = 1000000, mxx = -1000000, mxy = -1000000, cnt = 0;
    store_.for_each([&](int ix, int iy, Tile& tile) {
        if (tile.fresh) return;
        cnt++; mnx = std::min(mnx, ix); mny = std::min(mny, iy); mxx = std::max(mxx, ix); mxy = std::max(mxy, iy);
    });
    const int extent[4] = { cnt ? mnx : 0, cnt ? mny : 0, cnt ? mxx + 1 - mnx : 0, cnt ? mxy + 1 - mny : 0 };
    const int dims[4] = { w_, h_, off_x_, off_y_ };
    const double geo[6] = { min_[0], min_[1], max_[0], max_[1], ele_size_, length_pixel_ };
    pf_view_info v;
    const view::PlanResult pr = view::plan(V, width, height, level, dims, geo, band_num_ + 1, extent, &v);
    if (pr != view::kOk) return refuse(view::plan_message(pr));
    const size_t row = (size_t)width * channels, step = t.step ? t.step : row;
    if (t.kind != ViewTarget::Jpeg && step < row) return refuse("step is smaller than a row");
    if (t.kind == ViewTarget::Jpeg && !jpeg_size_ok(who, height, width)) return false;
    if (t.kind == ViewTarget::Device) {
        hipPointerAttribute_t at{};
        if (hipPointerGetAttributes(&at, t.out) != hipSuccess || at.type != hipMemoryTypeDevice || at.device != device_) {
            (void)hipGetLastError();
            return refuse("the destination is not memory of the map's device");
        }
    }
    Section sec(this, T_SAVE);
    for (auto& e : view_ev_) if (!e) HIP_OK(hipEventCreate(&e));
    const bool timed = view_timing_;
    // a caller's stream: its earlier work (a reader of the last view in the same buffer) goes first
    if (t.kind == ViewTarget::Device && t.has_stream) {
        HIP_OK(hipEventRecord(view_ev_[4], t.stream));
        HIP_OK(hipStreamWaitEvent(stream_, view_ev_[4], 0));
    }
    HIP_OK(sync_all());          // the tiles are read on stream_: every level stream has written them
    // where the kernels write: the caller's device memory, or a packed buffer of the map's on its way to the host or the encoder
    uint8_t* dev_out = t.out; size_t dev_step = step;
    if (t.kind != ViewTarget::Device) {
        if (!view_out_.reserve(row * height)) return false;
        dev_out = (uint8_t*)view_out_.p; dev_step = row;
    }
    if (timed) HIP_OK(hipEventRecord(view_ev_[0], stream_));
    if (v.empty) {
        if (timed) { HIP_OK(hipEventRecord(view_ev_[1], stream_)); HIP_OK(hipEventRecord(view_ev_[2], stream_)); }
        launch_view_fill(stream_, width, height, channels, opt_.bg_color, dev_out, dev_step);
    } else {
        const int k = v.level, wx = v.rect[2], wy = v.rect[3], e = kElePixels >> k, srows = wy * e, scols = wx * e;
        std::vector<uint64_t> tab((size_t)wx * wy, 0);          // absent tiles 0: zeros in the collapse, coverage 0
        for (int y = 0; y < wy; y++)
            for (int x = 0; x < wx; x++) {
                Tile* tile = store_.find(v.rect[0] + x, v.rect[1] + y);
                if (tile && !tile->fresh) tab[(size_t)y * wx + x] = (uint64_t)(uintptr_t)tile->base;
            }
        if (!view_table_.reserve(tab.size() * 8) || !view_bgr_.reserve((size_t)srows * scols * 3) || !view_cover_.reserve((size_t)srows * scols)) return false;
        HIP_OK(hipMemcpy(view_table_.p, tab.data(), tab.size() * 8, hipMemcpyHostToDevice));
        const uint64_t* table = (const uint64_t*)view_table_.p;
        if (k) launch_save_level(stream_, lay_, k, table, wx, wy, opt_.bg_color, (uint8_t*)view_bgr_.p);
        else launch_save_fused(stream_, lay_, table, wx, wy, opt_.bg_color, (uint8_t*)view_bgr_.p);
        if (timed) HIP_OK(hipEventRecord(view_ev_[1], stream_));
        launch_view_cover(stream_, table, wx, wy, k, lay_.w_off[k], (uint8_t*)view_cover_.p);
        if (timed) HIP_OK(hipEventRecord(view_ev_[2], stream_));
        launch_view_warp(stream_, (const uint8_t*)view_bgr_.p, (const uint8_t*)view_cover_.p, srows, scols, v.Minv, width, height, channels, opt_.bg_color, dev_out, dev_step);
    }
    if (timed) HIP_OK(hipEventRecord(view_ev_[3], stream_));
    HIP_OK(hipGetLastError());
    if (timed) {
        HIP_OK(hipEventSynchronize(view_ev_[3]));
        for (int i = 0; i < 3; i++) { float ms = 0; HIP_OK(hipEventElapsedTime(&ms, view_ev_[i], view_ev_[i + 1])); view_ms_[i] = ms; }
        view_ms_[3] = v.tiles;
    }
    if (t.kind == ViewTarget::Device) {
        if (t.has_stream) {          // the caller's stream goes on behind the view
            HIP_OK(hipEventRecord(view_ev_[5], stream_));
            HIP_OK(hipStreamWaitEvent(t.stream, view_ev_[5], 0));
        } else HIP_OK(hipStreamSynchronize(stream_));
    } else if (t.kind == ViewTarget::Host) {
        if (step == row) {
            if (!out_ring_.download(stream_, { OutPiece{ t.out, view_out_.p, row * height } })) return false;
        } else {                     // rows with padding between them: the padding keeps the caller's bytes
            std::vector<uint8_t> packed(row * height);
            if (!out_ring_.download(stream_, { OutPiece{ packed.data(), view_out_.p, packed.size() } })) return false;
            for (int y = 0; y < height; y++) std::memcpy(t.out + (size_t)y * step, packed.data() + (size_t)y * row, row);
        }
    } else {
        size_t off[2] = { 0, 0 };
        if (!jpeg_enc_.encode(view_out_.p, 1, nullptr, 0, height, width, row, t.quality, off, stream_)) return false;
        *t.len = off[1];
        if (off[1] > t.cap) {
            HIP_OK(hipStreamSynchronize(stream_));
            return refuse("the stream has " + std::to_string(off[1]) + " bytes, the buffer " + std::to_string(t.cap));
        }
        if (!jpeg_enc_.fetch(t.out, stream_)) return false;
    }
    if (info_out) *info_out = v;
    return true;
}

bool FusionMap::view_of_extent(int width, int height, double V[9])
{
    Drained l(*this);
    if (!valid_) { set_error("pf_view_of_extent: the map is not prepared"); return false; }
    int mnx = 1000000, mny = 1000000, mxx = -1000000, mxy = -1000000, cnt = 0;
    store_.for_each([&](int ix, int iy, Tile& tile) {
        if (tile.fresh) return;
        cnt++; mnx = std::min(mnx, ix); mny = std::min(mny, iy); mxx = std::max(mxx, ix); mxy = std::max(mxy, iy);
    });
    const int extent[4] = { mnx, mny, cnt ? mxx + 1 - mnx : 0, cnt ? mxy + 1 - mny : 0 };
    const int dims[4] = { w_, h_, off_x_, off_y_ };
    const double geo[6] = { min_[0], min_[1], max_[0], max_[1], ele_size_, length_pixel_ };
    if (!view::of_extent(dims, geo, extent, width, height, V)) { set_error("pf_view_of_extent: the map has no content, or a size that is not positive"); return false; }
    return true;
}

bool FusionMap::view_from_pose(const double pose_world7[7], const double* cam6, double V[9])
{
    std::lock_guard<std::mutex> l(mu_);          // geometry alone: nothing that waits is rendered
    if (!valid_) { set_error("pf_view_from_pose: the map is not prepared"); return false; }
    Camera c = cam_;
    if (cam6) {
        if (!(cam6[0] >= 1) || !(cam6[1] >= 1) || cam6[2] == 0 || cam6[3] == 0) { set_error("pf_view_from_pose: the camera needs w, h >= 1 and fx, fy != 0"); return false; }
        c = Camera{ cam6[0], cam6[1], cam6[2], cam6[3], cam6[4], cam6[5], 1. / cam6[2], 1. / cam6[3] };
    }
    if (!view::from_pose(c, mul(plane_inv_, pose_from7(pose_world7)), V)) { set_error("pf_view_from_pose: the pose looks at the plane too obliquely (feed would reject it)"); return false; }
    return true;
}

bool FusionMap::view_from_lnglat(const double gps_origin[3], double lng_w, double lat_n, double lng_e, double lat_s, int width, int height, double V[9])
{
    std::lock_guard<std::mutex> l(mu_);          // geometry alone
    if (!valid_) { set_error("pf_view_from_lnglat: the map is not prepared"); return false; }
    const double geo[6] = { min_[0], min_[1], max_[0], max_[1], ele_size_, length_pixel_ };
    double plane7[7];
    std::memcpy(plane7, plane_.t, 24); std::memcpy(plane7 + 3, plane_.q, 32);
    if (!view::from_lnglat(geo, plane7, gps_origin, lng_w, lat_n, lng_e, lat_s, width, height, V)) {
        set_error("pf_view_from_lnglat: a window without area, a size that is not positive or a georeference that is not finite");
        return false;
    }
    return true;
}

}  // namespace pf
