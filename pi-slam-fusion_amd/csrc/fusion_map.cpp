// fusion_map.cpp -- host engine: setup and teardown, and the render path -- renderFrame in stages, the cull, the lookahead, the
// launches -- following the control flow of Map2DFusion/MultiBandMap2DCPU.cpp.  The rest of the engine behind fusion_map.hpp:
// map_support.cpp (errors, timers, tile store, buffers, profiler), map_feed.cpp (prepare / feed / worker / sync), map_output.cpp
// (tile access, output ring, blend), map_save.cpp (save, web tiles), map_merge.cpp (map merge, state file).
#include "fusion_map.hpp"
#include "map_internal.hpp"
#include "env.hpp"
#include "warp_index.hpp"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace pf {

// ------------------------------------------------------------------ setup
FusionMap::FusionMap(int type, bool thread, const pf_options& opt) : opt_(opt), thread_(thread)
{
    // Map2D::create: TypeCPU -> Map2DCPU; TypeGPU falls back to Map2DCPU in the reference (Map2D.cpp:58-65)
    single_band_ = (type == PF_TYPE_CPU || type == PF_TYPE_GPU);
    const int lim = (int)std::ceil(std::log((double)kElePixels) / std::log(2.0));      // .cpp:263
    band_num_ = std::min(opt_.band_number, lim);
    if (band_num_ < 0) band_num_ = 0;
    if (single_band_) band_num_ = 0;
    lay_ = make_layout(band_num_, opt_.force_float != 0);
    if (single_band_) { lay_.f32 = 0; lay_.lap_off[0] = 0; lay_.w_off[0] = 0; lay_.slot_bytes = kElePixels * kElePixels * 4; }
    store_.configure(lay_.slot_bytes);
    if (opt_.max_queue <= 0) opt_.max_queue = 20;
    table_in_args_ = exp_env("PF_TABLE_COPY") == nullptr;              // experiments library, PF_TABLE_COPY=1: every tile table staged and copied in the stream (A/B, tests)
    if (opt_.shard_count < 1) opt_.shard_count = 1;
    if (opt_.shard_block < 1) opt_.shard_block = 8;
    opt_.lookahead = std::min(std::max(opt_.lookahead, 0), 64);

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        set_error("no HIP device: the fusion path has no CPU fallback");
        return;
    }
    if (opt_.device >= 0) device_ = opt_.device;
    else if (hipGetDevice(&device_) != hipSuccess) device_ = 0;
    if (device_ >= ndev) { set_error("device ordinal out of range"); return; }
    if (hipSetDevice(device_) != hipSuccess) { set_error("hipSetDevice failed"); return; }
    if (hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking) != hipSuccess) { set_error("hipStreamCreate failed"); return; }
    for (int i = 0; i < kTableRing; i++)
        if (hipEventCreateWithFlags(&table_ev_[i], hipEventDisableTiming) != hipSuccess) { set_error("hipEventCreate failed"); return; }
    for (int i = 0; i < kMarks; i++)
        if (hipEventCreateWithFlags(&mark_ev_[i], hipEventDisableTiming) != hipSuccess) { set_error("hipEventCreate failed"); return; }
    init_ok_ = true;
    if (thread_) worker_ = std::thread([this] { worker(); });
}

FusionMap::~FusionMap()
{
    if (worker_.joinable()) {
        { std::lock_guard<std::mutex> l(qmu_); stop_ = true; }
        qcv_.notify_all();
        worker_.join();
    }
    if (!init_ok_) return;
    (void)hipSetDevice(device_);
    (void)sync_all();
    prof_.harvest();
    for (int i = 0; i < kMaxLevels; i++) {
        bool shared = lvl_stream_[i] == stream_;
        for (int k = 1; k < i; k++) shared = shared || lvl_stream_[k] == lvl_stream_[i];
        if (i > 0 && lvl_stream_[i] && !shared) (void)hipStreamDestroy(lvl_stream_[i]);
        for (int k = 0; k < kLvlRing; k++) if (lvl_ev_[i][k]) (void)hipEventDestroy(lvl_ev_[i][k]);
    }
    for (auto& s : slots_) { if (s.dev) (void)hipFree(s.dev); if (s.consumed) (void)hipEventDestroy(s.consumed); }
    for (int i = 0; i < kTableRing; i++) {
        if (table_host_[i]) (void)hipHostFree(table_host_[i]);
        if (table_ev_[i]) (void)hipEventDestroy(table_ev_[i]);
        if (i < kMarks && mark_ev_[i]) (void)hipEventDestroy(mark_ev_[i]);
    }
    for (auto e : merge_ev_) if (e) (void)hipEventDestroy(e);
    for (auto e : view_ev_) if (e) (void)hipEventDestroy(e);
    jpeg_enc_.release(); deflate_enc_.release(); png_enc_.release(); tiff_dev_.release();
    (void)hipStreamDestroy(stream_);
    // the buffers (DevBuf), the tile store, the output ring and the profiler free what they hold as the members go, after this body: on
    // this thread, with the device current and nothing in flight.  None of them uses stream_
}

bool FusionMap::set_device() { HIP_OK(hipSetDevice(device_)); return true; }

// every stream this map launches on: the main stream (level 0, blend, save) and the
// per-level streams of the fused pipeline
hipError_t FusionMap::sync_all()
{
    if (!flush_pipeline()) return hipErrorUnknown;
    hipError_t e = hipStreamSynchronize(stream_);
    if (e == hipSuccess) synced_no_ = work_no_;
    for (int i = 1; i < kMaxLevels; i++)
        if (lvl_stream_[i] && lvl_stream_[i] != stream_) { hipError_t e2 = hipStreamSynchronize(lvl_stream_[i]); if (e == hipSuccess) e = e2; }
    return e;
}

// Allocator hint (no reference counterpart: the reference's tiles are cv::Mat on the heap): slabs for n more tiles
// are allocated and touched now, so that a mosaic of known extent never meets hipMalloc -- or the driver's
// page clearing behind it -- while keyframes are being fused.
bool FusionMap::reserve_tiles(long long n_tiles)
{
    std::lock_guard<std::mutex> l(mu_);
    if (!init_ok_ || n_tiles <= 0 || !set_device()) return false;
    std::vector<std::pair<char*, size_t>> fresh;
    if (!store_.reserve((size_t)n_tiles, &fresh)) return false;
    for (auto& f : fresh) HIP_OK(hipMemsetAsync(f.first, 0, f.second, stream_));
    HIP_OK(hipStreamSynchronize(stream_));
    return true;
}

void FusionMap::render_stats(double out[4])
{
    Drained l(*this);
    out[0] = (double)n_with_pixels_; out[1] = px_level0_; out[2] = px_owned_; out[3] = (double)store_.size();
}

void FusionMap::stats(long long* rendered, long long* rejected, long long* dropped, long long* failed)
{
    Drained l(*this);
    if (rendered) *rendered = n_rendered_;
    if (rejected) *rejected = n_rejected_;
    if (failed) *failed = n_failed_;
    std::lock_guard<std::mutex> q(qmu_);
    if (dropped) *dropped = n_dropped_;
}

// the tiles (dense index) a box of plane coordinates touches
void FusionMap::tile_range(double xmin, double ymin, double xmax, double ymax, Win& r) const
{
    r.x0 = (int)std::floor((xmin - min_[0]) * ele_size_inv_);
    r.y0 = (int)std::floor((ymin - min_[1]) * ele_size_inv_);
    r.x1 = (int)std::ceil((xmax - min_[0]) * ele_size_inv_);
    r.y1 = (int)std::ceil((ymax - min_[1]) * ele_size_inv_);
}

// 2. destination tile range of a footprint, spreadMap when it leaves the grid (.cpp:349-394)
bool FusionMap::canvas_range(const double pts[8], Win& r)
{
    double xmin = pts[0], xmax = xmin, ymin = pts[1], ymax = ymin;
    for (int i = 1; i < 4; i++) {
        if (pts[2 * i] < xmin) xmin = pts[2 * i];
        if (pts[2 * i + 1] < ymin) ymin = pts[2 * i + 1];
        if (pts[2 * i] > xmax) xmax = pts[2 * i];
        if (pts[2 * i + 1] > ymax) ymax = pts[2 * i + 1];
    }
    if (xmin < min_[0] || xmax > max_[0] || ymin < min_[1] || ymax > max_[1])
        if (!spread_map(xmin, ymin, xmax, ymax)) return false;
    tile_range(xmin, ymin, xmax, ymax, r);
    return true;
}

// spreadMap (.cpp:561-604): geometry only -- tiles live in a hash keyed by
// stable coordinates, so nothing is re-laid out.
bool FusionMap::spread_map(double xmin, double ymin, double xmax, double ymax)
{
    Section sec(this, T_SPREAD);
    Win r;
    tile_range(xmin, ymin, xmax, ymax, r);
    spread_tiles(r);
    return true;
}

void FusionMap::spread_tiles(const Win& r)
{
    const int xminInt = std::min(r.x0, 0), yminInt = std::min(r.y0, 0);
    const int xmaxInt = std::max(r.x1, w_), ymaxInt = std::max(r.y1, h_);
    const int w = xmaxInt - xminInt, h = ymaxInt - yminInt;
    const double mnx = min_[0] + ele_size_ * xminInt, mny = min_[1] + ele_size_ * yminInt;
    const double mxx = mnx + w * ele_size_, mxy = mny + h * ele_size_;
    min_[0] = mnx; min_[1] = mny; max_[0] = mxx; max_[1] = mxy;
    w_ = w; h_ = h; off_x_ += xminInt; off_y_ += yminInt;
}

// ------------------------------------------------------------ renderFrame
// MultiBandMap2DCPU::renderFrame (.cpp:311-558) in stages; FrameWork (fusion_map.hpp) is what one stage leaves for the next:
//   frame_canvas        1-3  footprint, tile range (canvas_range), homography          (.cpp:324-441)
//   build_tile_table         Apply's tile loop: owned tiles, the cull, the table entries (.cpp:476-492)
//   LevelPlan::windows / plan_fused_levels   where each pyramid level is needed: windows, compute regions, need bitmaps and rectangles
// The arithmetic of the plan -- the cull's bounds (Lattice) and the levels (LevelPlan) -- is frame_plan.hpp: pure, and checked on the CPU
// (tests/cpp/frame_plan_check.cpp).  Here: tiles, counters, the profiler and the launches around it.
//   reserve_frame_workspace / place_table   grow-only buffers, the table's ring slot
//   launch_fused_pipeline | launch_level_streams | launch_per_op | launch_single_band   the kernels (.cpp:443-555)
//   retire_frame             flags, weight bounds, counters
bool FusionMap::render_frame(const QueuedFrame& f)
{
    Section sec(this, T_RENDER);
    FrameWork& w = fw_;
    w.reset();
    // Geometry now, in feed order: the grid advances (spreadMap) and a keyframe is rejected inside its own feed call whether or not its
    // pixels wait for the lookahead.
    const int go = frame_canvas(f, w);
    if (go <= 0) { release_slot(f); if (go < 0) n_rejected_++; return go == 0; }          // -1: rejected (.cpp:340-343, :381-386); 0: geometry-only frame
    pending_.emplace_back();
    PendingFrame& p = pending_.back();
    p.f = f;
    std::memcpy(p.pts, w.pts, sizeof(p.pts));
    p.sx0 = w.xminInt + off_x_; p.sy0 = w.yminInt + off_y_; p.tx = w.tx; p.ty = w.ty;
    std::memcpy(p.M0, w.M0, sizeof(p.M0));
    // may this keyframe's cells be culled?  (the lattice of its canvas mapped into the source, if so)
    w.cull = cull_on_ && (single_band_ || (opt_.fused == 1 && w.L >= 1)) && invert3x3(w.M0, w.Minv) && cull_frame_ok(w.Minv, w.crows, w.ccols);
    p.cull = w.cull;
    std::memcpy(p.Minv, w.Minv, sizeof(p.Minv));
    if (f.slot >= 0) { std::lock_guard<std::mutex> q(qmu_); slots_[f.slot].queued = true; }      // held until the keyframe is rendered (retire_frame)
    size_t keep = 0;
    if (w.cull) {
        if (!lat_pool_.empty()) { p.lat = std::move(lat_pool_.back()); lat_pool_.pop_back(); }
        w.lat = &p.lat;
        // a shard that owns a quarter of the canvas' tiles or more has the whole lattice mapped at once, like an unsharded map (one tile_owner
        // call per tile: ~1 us); below that the points are mapped as its tiles ask for them
        bool map_all = opt_.shard_count <= 1;
        if (!map_all) {
            int mine = 0;
            for (int y = 0; y < w.ty; y++)
                for (int x = 0; x < w.tx; x++) mine += tile_owner(opt_.shard_count, opt_.shard_block, w.xminInt + x + off_x_, w.yminInt + y + off_y_) == opt_.shard_rank;
            map_all = 4 * mine >= w.tx * w.ty;
        }
        // multi-band: the bounds over the cell itself, widened by the pyramid's slack (build_tile_table has the argument); only the test
        // that a lower bound's support lies inside the frame keeps the pyramid's reach, 2^(L+1) - 2 pixels rounded up to lattice steps.
        // Experiments library, PF_CULL_DILATED=1: both bounds over the cell dilated by that reach and no slack (the rule before; A/B, tests)
        static const bool dilated_rule = exp_env("PF_CULL_DILATED") != nullptr;
        const int reach = single_band_ ? 0 : ((2 << w.L) - 2 + 63) / 64;
        if (single_band_ || dilated_rule) p.lat.map_canvas(w.Minv, w.crows, w.ccols, f.cols, f.rows, reach, map_all, cull_margins_);
        else {
            const double far = 64.0 * reach, s = map_lipschitz(w.Minv, -far, w.ccols + far, -far, w.crows + far);
            p.lat.map_canvas(w.Minv, w.crows, w.ccols, f.cols, f.rows, 0, map_all, cull_margins_, reach, pyramid_slack(s, w.L));
        }
        if (lookahead_ok()) {
            // the keyframe's own lower bounds enter the tiles' wlb NOW: the keyframes ahead of it in the queue are decided against them
            if (!tiles_pool_.empty()) { p.tiles = std::move(tiles_pool_.back()); tiles_pool_.pop_back(); }
            // From here on later keyframes are culled against this one, so whatever of its render can fail for want of memory is done first:
            // the workspace of its canvas, then its tiles.  A failure loses this keyframe inside its own feed call, as without a lookahead,
            // and nothing of it is in any wlb
            if (!reserve_frame_workspace(w) || !pre_raise(w, p.tiles)) {
                if (p.lat.sx.capacity() && lat_pool_.size() < 8) lat_pool_.push_back(std::move(p.lat));
                if (p.tiles.capacity() && tiles_pool_.size() < 8) tiles_pool_.push_back(std::move(p.tiles));
                pending_.pop_back();
                release_slot(f);
                keyframe_lost();
                return false;
            }
            p.pre_raised = true;
            since_drain_++;
            keep = std::min<size_t>((size_t)opt_.lookahead, 2 * (size_t)since_drain_ / 3);
        }
    }
    // a keyframe that cannot take part (no cull for it: an untame homography, a per-level or per-op map, the cull switched off) is rendered at
    // once, and everything that waits before it; a failure of one of THOSE renders is reported by this call
    while (pending_.size() > keep)
        if (!render_front()) return false;
    return true;
}

// The weight bounds of an admitted keyframe go into its tiles' wlb (Lattice::raise_bounds; build_tile_table does not work them out again).
// Creates the canvas' tiles, as Apply's tile loop does (.cpp:478-492), and remembers them for the render.  All tiles first, then the bounds:
// when the store cannot grow (false; the tiles made so far stay, fresh) no wlb holds a bound of a keyframe that will not be rendered.
bool FusionMap::pre_raise(FrameWork& w, std::vector<Tile*>& tiles)
{
    tiles.assign((size_t)w.tx * w.ty, nullptr);
    const bool sharded = opt_.shard_count > 1;
    for (int y = 0; y < w.ty; y++)
        for (int x = 0; x < w.tx; x++) {
            const int sx = w.xminInt + x + off_x_, sy = w.yminInt + y + off_y_;
            if (sharded && tile_owner(opt_.shard_count, opt_.shard_block, sx, sy) != opt_.shard_rank) continue;
            Tile* t = store_.get_or_create(sx, sy);
            if (!t) { tiles.clear(); return false; }          // HBM exhausted
            tiles[(size_t)y * w.tx + x] = t;                  // (references into the store stay valid while it grows)
        }
    for (int y = 0; y < w.ty; y++)
        for (int x = 0; x < w.tx; x++)
            if (Tile* t = tiles[(size_t)y * w.tx + x]) w.lat->raise_bounds(x, y, opt_.weight_type, t->wlb);
    return true;
}

void FusionMap::release_slot(const QueuedFrame& f)
{
    if (f.slot < 0) return;
    std::lock_guard<std::mutex> q(qmu_);
    slots_[f.slot].queued = false;
}

bool FusionMap::drain()
{
    since_drain_ = 0;
    if (pending_.empty()) return true;
    if (!set_device()) return false;
    // (a keyframe that fails costs that keyframe: the others that wait are rendered all the same, or a reader -- which has no use for
    // the result -- would look at a map short of them too)
    bool ok = true;
    while (!pending_.empty()) ok = render_front() && ok;
    return ok;
}

// stages 4 onwards of renderFrame for the oldest keyframe that waits.  When they fail the keyframe is lost, and counted: keyframes admitted
// after it may have been culled against its bounds (reserve_frame_workspace and the tiles are seen to at admission for that reason; what is
// left is the launches themselves and the one-off weight plane), so the caller of this call or of the next sync() has to hear of it
bool FusionMap::render_front()
{
    const bool ok = render_front_stages();
    if (!ok) keyframe_lost();
    return ok;
}

bool FusionMap::render_front_stages()
{
    struct Pop {            // the keyframe leaves the queue whatever happens to it (its lattice's buffers go back to the pool)
        FusionMap* m;
        ~Pop() {
            PendingFrame& p = m->pending_.front();
            if (p.lat.sx.capacity() && m->lat_pool_.size() < 8) m->lat_pool_.push_back(std::move(p.lat));
            if (p.tiles.capacity() && m->tiles_pool_.size() < 8) m->tiles_pool_.push_back(std::move(p.tiles));
            m->pending_.pop_front();
        }
    } pop{ this };
    PendingFrame& p = pending_.front();
    const QueuedFrame f = p.f;
    struct Held { FusionMap* m; const QueuedFrame& f; bool done = false; ~Held() { if (!done) m->release_slot(f); } } held{ this, f };
    FrameWork& w = fw_;
    w.reset();
    std::memcpy(w.pts, p.pts, sizeof(p.pts));
    w.xminInt = p.sx0 - off_x_; w.yminInt = p.sy0 - off_y_; w.xmaxInt = w.xminInt + p.tx; w.ymaxInt = w.yminInt + p.ty;
    w.tx = p.tx; w.ty = p.ty; w.L = band_num_; w.crows = w.ty * kElePixels; w.ccols = w.tx * kElePixels;
    std::memcpy(w.M0, p.M0, sizeof(p.M0)); std::memcpy(w.Minv, p.Minv, sizeof(p.Minv));
    w.cull = p.cull;
    w.pre_raised = p.pre_raised;
    w.tiles_known = p.tiles.size() == (size_t)p.tx * p.ty ? p.tiles.data() : nullptr;
    if (w.pre_raised && !w.tiles_known) { set_error("render_front: a keyframe admitted without its tiles"); return false; }      // (render_frame admits none)
    w.src = f.ext ? f.ext : slots_[f.slot].dev;
    w.lat = &p.lat;
    Section sec_apply(this, T_APPLY);          // the reference times its tile loop under this name (.cpp:476-555); here: table, need rectangles, launch
    if (!build_tile_table(f, w)) return false;
    if (w.bx0 >= w.bx1) {                      // nothing of this frame lands on this shard, or it cannot win anywhere it lands
        for (auto& r : w.raise) r.t->wlb[r.q] = std::max(r.t->wlb[r.q], r.w);
        for (Tile* t : w.culled) t->changed = true;
        if (w.owned_all) n_rendered_++;
        log_rendered(f);
        return true;
    }
    px_owned_ += (double)w.owned * kElePixels * kElePixels;     // what this rank renders beyond its share: owned tile pixels vs the level-0 window (bench --shard strong)
    n_with_pixels_++;
    w.plan.windows(w.pb, w.L, w.crows, w.ccols);
    if (!reserve_frame_workspace(w) || !place_table(w)) return false;
    warp_args(f, w);
    const bool fused = opt_.fused != 0 && w.L >= 1;
    bool ok;
    if (single_band_) ok = launch_single_band(f, w);
    else if (fused) {
        // weightImage (MultiBandMap2DCPU.cpp:396-425): built once per frame size, gathered by the warp
        if (wmap_rows_ != f.rows || wmap_cols_ != f.cols) {
            HIP_OK(sync_all());
            if (!wmap_.reserve((size_t)f.rows * f.cols * 4)) return false;
            launch_weight32(stream_, (float*)wmap_.p, f.rows, f.cols, opt_.weight_type);
            wmap_rows_ = f.rows; wmap_cols_ = f.cols;
        }
        w.a.wmap = (const float*)wmap_.p;
        plan_fused_levels(w);
        ok = opt_.fused == 1 ? launch_fused_pipeline(f, w) : launch_level_streams(f, w);
    } else ok = launch_per_op(f, w);
    if (!ok) return false;
    HIP_OK(hipGetLastError());
    held.done = true;                          // retire_frame hands the slot over to its consumed event
    return retire_frame(f, w, fused);
}

void FusionMap::log_rendered(const QueuedFrame& f)
{
    if (f.seq < 0) return;
    if (render_log_.size() >= 65536) render_log_.erase(render_log_.begin(), render_log_.begin() + 32768);
    render_log_.push_back(f.seq);
}

// 1. pose -> ground points (.cpp:324-347); 2. destination tile range, spreadMap when the footprint leaves the grid (.cpp:349-394);
// 3. homography (.cpp:427-441).  Returns 1 to go on, 0 for a geometry-only frame (other shards own its tiles), -1 rejected.
int FusionMap::frame_canvas(const QueuedFrame& f, FrameWork& w)
{
    double* pts = w.pts;
    if (!footprint(cam_, f.pose, pts)) return -1;
    Win r;
    if (!canvas_range(pts, r)) return -1;
    w.xminInt = r.x0; w.yminInt = r.y0; w.xmaxInt = r.x1; w.ymaxInt = r.y1;
    if (w.xminInt < 0 || w.yminInt < 0 || w.xmaxInt > w_ || w.ymaxInt > h_ || w.xminInt >= w.xmaxInt || w.yminInt >= w.ymaxInt) {
        std::fprintf(stderr, "MultiBandMap2DCPU::renderFrame:should never happen!\n");
        return -1;
    }
    const double xmin = min_[0] + ele_size_ * w.xminInt, ymin = min_[1] + ele_size_ * w.yminInt;
    w.src = f.ext ? f.ext : (f.slot >= 0 ? slots_[f.slot].dev : nullptr);
    if (!w.src) return 0;
    const float src4[8] = { 0.f, 0.f, (float)cam_.w, 0.f, 0.f, (float)cam_.h, (float)cam_.w, (float)cam_.h };
    float dst4[8];
    for (int i = 0; i < 4; i++) {
        dst4[2 * i]     = (float)((pts[2 * i] - xmin) * length_pixel_inv_);
        dst4[2 * i + 1] = (float)((pts[2 * i + 1] - ymin) * length_pixel_inv_);
    }
    perspective_transform(src4, dst4, w.M0);
#if PF_EXPERIMENTS
    if (!next_M0_.empty()) { std::memcpy(w.M0, next_M0_.front().m, sizeof(w.M0)); next_M0_.pop_front(); }       // debug_next_homography()
#endif
    w.tx = w.xmaxInt - w.xminInt; w.ty = w.ymaxInt - w.yminInt; w.L = band_num_;
    w.crows = w.ty * kElePixels; w.ccols = w.tx * kElePixels;
    return 1;
}

// One pass over the canvas tiles (Apply's tile loop, .cpp:478-492): the tiles this shard owns, their bounding box,
// the hash cells they fall in (for the need rectangles) and the table entries: slot address | fresh bit | culled cells.
// The reference's own per-frame O(tiles) cost is d->data() at .cpp:477.
//
// Cull (round 4): a cell of a tile in which this keyframe cannot win the max-weight select at ANY level is left out of the launch -- a
// tile whose cells are all out keeps table entry 0, exactly as if another shard owned it, and the level-0 blocks' own need test / the
// need rectangles shrink the grid to what the remaining cells depend on.  Nothing changes in what is stored: `if (srcW >= dstW)`
// (.cpp:521, :542) is false at every pixel of such a cell.  Sound because both sides are bounded from the geometry alone, with margins
// (cell_out):
//   the weights   A pixel p of level i belongs to the cell that holds its level-0 position 2^i p.  Its weight W_i(p) is the level-0 weight
//                 image v under the i-fold composition of pyrDown's [1 4 6 4 1] / 16: a convex combination of v centred on 2^i p with
//                 variance (4^i - 1) / 3 per axis (BORDER_REFLECT_101 only folds positions towards the inside of the canvas), so
//                 E |x - 2^i p| <= sqrt(2 (4^L - 1) / 3) =: rms (26 px for five bands, 104 for seven).  v(x) is a radial weight of the
//                 source pixel H(x) -- Lipschitz in its distance from the image centre with constant 1 / dis_max -- or 0 outside the
//                 frame, and H is Lipschitz on the canvas with constant s (map_lipschitz).  With S = s rms (pyramid_slack):
//   new weights   W_i(p) <= max(radial weight at 2^i p, floor) + S / dis_max <= the weight at distance dist(centre, H(cell)) - S
//                 (the zeros outside the frame only lower W; squared weights: E (w + t)^2 <= (w + S / dis_max)^2 as E t^2 <= (S / dis_max)^2);
//   stored ones   every earlier keyframe f whose canvas held the tile left S_i >= W_i^f >= wmin_f = the weight at distance
//                 (farthest corner of H_f(cell)) + S_f, provided every point of the combination maps inside f's frame -- the cell
//                 dilated by the pyramid's support radius 2^(L+1) - 2 pixels, rounded up to lattice steps, does -- and 0 otherwise
//                 (squared weights: Jensen); also when f itself was culled there, for then S_i > W_i^f.
//                 Tile::wlb[cell] = max over f of wmin_f.
// Only the support of the combination entered the rule before this one (both bounds over the dilated cell: 192 x 192 px for five bands;
// experiments library, PF_CULL_DILATED=1); its concentration is what S uses.  Both are checked against the weights themselves on the host
// (tests/cpp/cull_slack_check.cpp, frame_plan_check.cpp).
// Bit-exactness is checked, not assumed: every parity test runs with the cull on; PF_CULL=0 turns it off.
// The unit of the cull is a CELL of a tile (64 x 64 pixels, 16 per tile; experiments library, PF_CULL_SUB=2: a quadrant).  A tile whose
// cells are all out is left out of the launch; otherwise the cells that are out travel as flag bits of its table entry and the kernels do
// not look at their pixels (kernels.hip, cell_culled), which may have been computed from input nobody produced.
bool FusionMap::build_tile_table(const QueuedFrame& f, FrameWork& w)
{
    const int tx = w.tx, ty = w.ty;
    w.sharded = opt_.shard_count > 1;
    const bool sharded = w.sharded;
    const bool cull = w.cull;                                    // decided when the keyframe was admitted (render_frame), with its lattice (w.lat)
    const bool lookahead = cull && lookahead_ok();
    if (cull) w.raise.reserve((size_t)tx * ty * cull_margins_.sub * cull_margins_.sub);
    const int B = opt_.shard_block;
    // cells of the need rectangles: a shard's hash cells; for the cull alone squares of 8 x 8 tiles as well (experiments library: PF_CULL_CELL)
    static const int bc_env = exp_env_int("PF_CULL_CELL", 0);
    const int Bc = sharded ? B : (bc_env > 0 ? bc_env : 8);      // measured (profiles/r04_ab.md): 8 beats 3 / 4 (fewer, tighter-merging rectangles; less host work)
    table_tmp_.resize((size_t)tx * ty);
    w.touched.reserve((size_t)tx * ty);
    w.bx0 = tx; w.bx1 = 0; w.by0 = ty; w.by1 = 0;
    // the same box in level-0 pixels, around the cells that are rendered (== the tiles' box when nothing is culled); the squares of the rectangles likewise
    w.pb = Win{ 1 << 30, 0, 1 << 30, 0 };
    auto add_rect = [&](int sx, int sy, int x0, int y0, int x1, int y1) {
        w.pb.x0 = std::min(w.pb.x0, x0); w.pb.x1 = std::max(w.pb.x1, x1); w.pb.y0 = std::min(w.pb.y0, y0); w.pb.y1 = std::max(w.pb.y1, y1);
        if (sharded || cull) w.cells.add(floordiv(sx, Bc), floordiv(sy, Bc), x0, y0, x1, y1);
    };
    for (int y = 0; y < ty; y++) {
        const int sy = w.yminInt + y + off_y_;
        for (int x = 0; x < tx; x++) {
            const int sx = w.xminInt + x + off_x_;
            uint64_t ent = 0;
            Tile* known = w.tiles_known ? w.tiles_known[(size_t)y * tx + x] : nullptr;
            if (known || ((!sharded || tile_owner(opt_.shard_count, B, sx, sy) == opt_.shard_rank) && !w.tiles_known)) {
                Tile* t = known ? known : store_.get_or_create(sx, sy);
                if (!t) return false;
                w.owned_all++;
                unsigned out = 0;                                  // 64 x 64 cells in which this keyframe cannot win (bit 4 * row + column)
                if (cull) {
                    // the whole tile, then cell by cell; a fresh tile is rendered whole or not at all (Lattice::tile_cull)
                    TileCull c;
                    w.lat->tile_cull(x, y, t->wlb, t->fresh, lookahead, w.pre_raised, opt_.weight_type, single_band_, c);
                    out = c.out;
                    for (int k = 0; k < c.nraise; k++) w.raise.push_back(FrameWork::Raise{ t, c.q[k], c.w[k] });
                    if (out == 0xffffu && t->fresh) {
                        // stays fresh, and is not yet a tile of the mosaic (no Ischanged: it has no pyramid, .cpp:717-718)
                        w.culled_any = true; table_tmp_[(size_t)y * tx + x] = 0; n_culled_tiles_++;
                        continue;
                    }
                    if (out == 0xffffu) {
                        // not rendered, but still a tile of this keyframe's canvas: Apply sets Ischanged on every one of them
                        // (.cpp:553), and draw() re-blends it with whatever its neighbours have become
                        w.culled_any = true; table_tmp_[(size_t)y * tx + x] = 0; n_culled_tiles_++; w.culled.push_back(t);
                        continue;
                    }
                    if (out) { w.culled_any = true; n_culled_cells_ += __builtin_popcount(out); }
                }
                if ((uint64_t)(uintptr_t)t->base >> 48) { set_error("tile slot address above 2^48: the table entry has no room for the cell flags"); return false; }
                ent = (uint64_t)(uintptr_t)t->base | (t->fresh ? 1u : 0u) | ((uint64_t)out << 48);
                w.touched.push_back(t);
                w.owned++;
                w.bx0 = std::min(w.bx0, x); w.bx1 = std::max(w.bx1, x + 1); w.by0 = std::min(w.by0, y); w.by1 = std::max(w.by1, y + 1);
                if (!out) add_rect(sx, sy, x * kElePixels, y * kElePixels, (x + 1) * kElePixels, (y + 1) * kElePixels);
                else
                    for (int r = 0; r < 4; r++) {                  // the rendered cells, row by row as runs
                        const unsigned in = ~(out >> (4 * r)) & 15u;
                        if (!in) continue;
                        const int c0 = __builtin_ctz(in), c1 = 32 - __builtin_clz(in);
                        add_rect(sx, sy, x * kElePixels + 64 * c0, y * kElePixels + 64 * r, x * kElePixels + 64 * c1, y * kElePixels + 64 * r + 64);
                    }
            }
            table_tmp_[(size_t)y * tx + x] = ent;
        }
    }
    return true;
}

// grow-only workspace: per-frame Gaussian levels (GW_i of the fused forms, G_i / W_i of the per-op form) and the tile-table ring
bool FusionMap::reserve_frame_workspace(FrameWork& w)
{
    const int L = w.L, tx = w.tx, ty = w.ty;
    const size_t es = lay_.f32 ? 4 : 2;
    const bool fused = opt_.fused != 0 && L >= 1;
    const size_t pxb = level_px_bytes(lay_.f32 != 0);
    bool grow = false;
    for (int i = 0; i <= L; i++) {
        const size_t n = (size_t)(w.crows >> i) * (w.ccols >> i);
        if (single_band_) continue;
        if (fused) { if (i >= 1 && i < L && (gw_[i].cap < n * pxb || gw2_[i].cap < n * pxb)) grow = true; }
        else if (g_[i].cap < n * 3 * es || wgt_[i].cap < n * 4) grow = true;
    }
    if (table_cap_ < (size_t)tx * ty) grow = true;
#if PF_EXPERIMENTS
    if (dbg_fail_workspace_ > 0) {
        // debug_fail_workspace(): this call meets a hipMalloc that refuses -- 2^60 bytes asked of the first buffer of the workspace, which
        // goes the way DevBuf::reserve sends a buffer that cannot grow (released; the next call that needs it allocates it again)
        dbg_fail_workspace_--;
        HIP_OK(sync_all());
        DevBuf& b = single_band_ ? table_dev_[0] : (fused ? gw_[1] : g_[0]);
        if (&b == &table_dev_[0]) table_cap_ = 0;
        return b.reserve((size_t)1 << 60);
    }
#endif
    if (!grow) return true;
    HIP_OK(sync_all());
    for (int i = 0; i <= L; i++) {
        const size_t n = (size_t)(w.crows >> i) * (w.ccols >> i);
        if (single_band_) continue;
        if (fused) { if (i >= 1 && i < L && (!gw_[i].reserve(n * pxb) || !gw2_[i].reserve(n * pxb))) return false; }
        else if (!g_[i].reserve(n * 3 * es) || !wgt_[i].reserve(n * 4)) return false;
    }
    if (table_cap_ < (size_t)tx * ty) {
        table_cap_ = (size_t)tx * ty * 2;
        for (int i = 0; i < kTableRing; i++) {
            if (table_host_[i]) (void)hipHostFree(table_host_[i]);
            HIP_OK(hipHostMalloc((void**)&table_host_[i], table_cap_ * 8, hipHostMallocDefault));
            if (!table_dev_[i].reserve(table_cap_ * 8)) return false;
            table_pending_[i] = false;
        }
    }
    return true;
}

// the frame's tile table -> ring slot in device memory: inside the kernel arguments of the pipelined launch (which stores it there
// itself), or staged in pinned memory and copied in the stream
bool FusionMap::place_table(FrameWork& w)
{
    const int tx = w.tx, ty = w.ty;
    w.ring = (int)(frame_seq_++ % kTableRing);
    const int ring = w.ring;
    if (table_pending_[ring]) { HIP_OK(hipEventSynchronize(table_ev_[ring])); table_pending_[ring] = false; }
    w.table_args = table_in_args_ && opt_.fused == 1 && !single_band_ && w.L >= 2 && (size_t)tx * ty <= (size_t)kArgTable;
    if (!w.table_args) {
        // staged in pinned memory and copied in the stream; the staging slot is reused once that copy has run
        if (!wait_for(table_release_[ring])) return false;
        std::memcpy(table_host_[ring], table_tmp_.data(), (size_t)tx * ty * 8);
        HIP_OK(hipMemcpyAsync(table_dev_[ring].p, table_host_[ring], (size_t)tx * ty * 8, hipMemcpyHostToDevice, stream_));
    }
    w.dtab = (const uint64_t*)table_dev_[ring].p;
    return true;
}

// warp (.cpp:443-452): destination -> source map, window, radial weight constants
void FusionMap::warp_args(const QueuedFrame& f, FrameWork& w)
{
    WarpArgs& a = w.a;
    a = WarpArgs{};
    if (!invert3x3(w.M0, a.M)) std::memset(a.M, 0, sizeof(a.M));
    a.srows = f.rows; a.scols = f.cols; a.sstep = f.step;
    a.crows = w.crows; a.ccols = w.ccols;
    const Win& n0 = w.plan.need[0];
    a.y_off = n0.y0; a.x_off = n0.x0; a.wrows = n0.y1 - n0.y0; a.wcols = n0.x1 - n0.x0;
    a.xc = (float)(f.cols / 2); a.yc = (float)(f.rows / 2);
    a.dis_max = std::sqrt(a.xc * a.xc + a.yc * a.yc);
    a.weight_type = opt_.weight_type;
    a.src_cn = f.cn == 4 ? 4 : 3;
}

// Map2DCPU::renderFrame (Map2DCPU.cpp:236-334): per-pixel work only, so a shard needs no halo
bool FusionMap::launch_single_band(const QueuedFrame& f, FrameWork& w)
{
    WarpArgs& a = w.a;
    if (w8_rows_ != f.rows || w8_cols_ != f.cols) {
        HIP_OK(sync_all());
        if (!w8_.reserve((size_t)f.rows * f.cols)) return false;
        launch_weight8(stream_, (uint8_t*)w8_.p, f.rows, f.cols, opt_.weight_type);
        w8_rows_ = f.rows; w8_cols_ = f.cols;
    }
    a.y_off = w.by0 * kElePixels; a.x_off = w.bx0 * kElePixels;
    a.wrows = (w.by1 - w.by0) * kElePixels; a.wcols = (w.bx1 - w.bx0) * kElePixels;
    prof_begin(K_SINGLE, (double)a.src_cn * f.rows * f.cols + (double)a.wrows * a.wcols * 8);
    launch_single(stream_, w.src, (const uint8_t*)w8_.p, a, w.dtab, w.tx);
    prof_end();
    return true;
}

// Fused forms: where the level kernels run (LevelPlan, frame_plan.hpp), and the level-0 pixels that costs (render_stats)
void FusionMap::plan_fused_levels(FrameWork& w)
{
    const int BHr = level_block_rows(lay_.f32 != 0);
    // (the level-0 job carries rectangles wherever the plan consults the reach)
    const bool rects = w.plan.plan(table_tmp_.data(), w.tx, w.ty, w.L, w.pb, w.cells, w.sharded, w.culled_any, opt_.fused, BHr,
                                   level0_need_reach(lay_, w.table_args ? w.tx * w.ty : 0, 1));
    if (rects && w.plan.merged) count_merged_plan();
    const Win& C0 = w.plan.C[0];
    px_level0_ += rects ? w.plan.blocks_run0 * 64 * BHr : (double)(C0.x1 - C0.x0) * (C0.y1 - C0.y0);
#if PF_EXPERIMENTS
    static const bool exact_stat = exp_env("PF_CULL_EXACT_STAT") != nullptr;
    if (rects && exact_stat) cull_exact_stat(w);
#endif
}

// fused = 1: one launch per keyframe -- this frame's level 0 plus the pending upper levels of the frames before it
bool FusionMap::launch_fused_pipeline(const QueuedFrame& f, FrameWork& w)
{
    const int L = w.L;
    const size_t es = lay_.f32 ? 4 : 2;
    const double E = 3 * es + 4, owned_tiles = w.owned_all;       // algorithmic bytes: every canvas tile of this rank, culled or not
    double run_share[kMaxLevels];
    int exact_r0 = 0;
    LevelPlan& pl = w.plan;
    pl.run_shares(w.owned_all, prof_would(K_LEVEL0), run_share, &exact_r0);
    PipeFrame cur;
    cur.valid = true; cur.ring = w.ring; cur.tx = w.tx; cur.crows = w.crows; cur.ccols = w.ccols;
    for (int i = 0; i < L; i++) {
        cur.C[i] = pl.C[i]; cur.nrect[i] = pl.nrect[i];
        for (int k = 0; k < pl.nrect[i]; k++) cur.rect[i][k] = pl.rects[i][k];
        const double ts = kElePixels >> i, n = owned_tiles * ts * ts;
        // algorithmic bytes: frame read once + per tile-level pixel 4 (stored weight) + E (payload)
        const double tile_bytes = n * (4 + E) + (i + 1 == L ? n / 4 * (4 + E) : 0), frame_bytes_read = i == 0 ? (double)w.a.src_cn * f.rows * f.cols : 0;
        cur.bytes[i] = tile_bytes + frame_bytes_read;                         // every canvas tile of this rank, culled or not
        cur.bytes_run[i] = tile_bytes * run_share[i] + frame_bytes_read;      // the part of the canvas whose blocks run
    }
    if (w.table_args) { cur.table_args = table_tmp_.data(); cur.table_n = w.tx * w.ty; }
    for (int i = 1; i < L; i++) { cur.need_n[i] = pl.need_n[i]; if (pl.need_n[i] > 0) std::memcpy(cur.need_bits[i], pl.need_bits[i], sizeof(uint32_t) * (size_t)((pl.need_n[i] + 31) / 32)); }
    if (!launch_pipeline(&cur, &w.a, w.src)) return false;
    if (double* rec_bytes_run = exact_r0 > 0 ? prof_.last_bytes_run() : nullptr) {
        // this launch is bracketed by events: replace the level-0 job's estimated run share in its record by the exact one -- now that
        // the launch is on its way
        const double n0 = owned_tiles * kElePixels * kElePixels, tile_bytes0 = n0 * (4 + E) + (L == 1 ? n0 / 4 * (4 + E) : 0);
        *rec_bytes_run += tile_bytes0 * (pl.exact_level0_share(w.owned_all, exact_r0) - run_share[0]);
    }
    return true;
}

// fused = 2 / 3: one launch per level, level 0 on stream_ and the upper levels on kUpperStreams more.
// Level i of frame f runs after level i-1 of frame f (GW_i, event) and, by stream order, after level i of
// frame f-1 (tiles are updated in feed order).  GW buffers are double-buffered by frame parity; a writer
// waits for the reader two frames back.
bool FusionMap::launch_level_streams(const QueuedFrame& f, FrameWork& w)
{
    const int L = w.L;
    const size_t es = lay_.f32 ? 4 : 2;
    const double E = 3 * es + 4;
    const Win* C = w.plan.C;
    const unsigned long long fidx = frame_seq_ - 1;
    const int slot = (int)(fidx % kLvlRing);
    DevBuf* gw = (fidx & 1) ? gw2_ : gw_;
    for (int i = 0; i < L; i++) {
        if (!lvl_stream_[i]) {
            // HIP multiplexes streams onto a few hardware queues (4 by default), and streams that share one
            // serialize: keep the count small.  Level 0 has its own stream, the upper levels -- a dependent
            // chain within a frame anyway -- share kUpperStreams (experiments library: PF_LEVEL_STREAMS, PF_SINGLE_STREAM).
            static const int n_upper = exp_env_int("PF_LEVEL_STREAMS", kUpperStreams);
            if (i == 0) lvl_stream_[0] = stream_;
            else if (exp_env("PF_SINGLE_STREAM") || n_upper <= 0) lvl_stream_[i] = stream_;      // diagnostics: serial kernel times
            else if (i > n_upper) lvl_stream_[i] = lvl_stream_[1 + (i - 1) % n_upper];
            else HIP_OK(hipStreamCreateWithFlags(&lvl_stream_[i], hipStreamNonBlocking));
        }
        for (int k = 0; k < kLvlRing; k++)
            if (!lvl_ev_[i][k]) HIP_OK(hipEventCreateWithFlags(&lvl_ev_[i][k], hipEventDisableTiming));
    }
    for (int i = 0; i < L; i++) {
        hipStream_t st = lvl_stream_[i];
        const double ts = kElePixels >> i, n = (double)(w.bx1 - w.bx0) * (w.by1 - w.by0) * ts * ts;
        const bool top = (i + 1 == L);
        if (i > 0) HIP_OK(hipStreamWaitEvent(st, lvl_ev_[i - 1][slot], 0));
        if (!top && fidx >= 2) HIP_OK(hipStreamWaitEvent(st, lvl_ev_[i + 1][(int)((fidx - 2) % kLvlRing)], 0));
        // algorithmic bytes: frame read once + per tile-level pixel 4 (stored weight) + E (payload)
        double bytes = n * (4 + E) + (top ? n / 4 * (4 + E) : 0);
        if (i == 0) bytes += (double)w.a.src_cn * f.rows * f.cols;
        prof_begin(i == 0 ? K_LEVEL0 : K_LEVEL, bytes, st);
        launch_level(st, lay_, i, w.crows >> i, w.ccols >> i, C[i].x0, C[i].y0, C[i].x1, C[i].y1, w.tx, top, !top,
                     i == 0 ? &w.a : nullptr, w.src, i == 0 ? nullptr : gw[i].p, top ? nullptr : gw[i + 1].p, w.dtab, opt_.fused);   // 2: 4-stage k_level, 3: k_level3
        prof_end();
        HIP_OK(hipEventRecord(lvl_ev_[i][slot], st));
    }
    // the tile table of this ring slot is read until the last level has run
    HIP_OK(hipEventRecord(table_ev_[w.ring], lvl_stream_[L - 1]));
    table_pending_[w.ring] = true;
    return true;
}

// fused = 0: one kernel per reference op -- warp (.cpp:443-452), the Gaussian pyramids (.cpp:469 first loop, .cpp:471-474),
// Laplacian + select into tiles (.cpp:469 second loop, .cpp:476-555)
bool FusionMap::launch_per_op(const QueuedFrame& f, FrameWork& w)
{
    const int L = w.L;
    const size_t es = lay_.f32 ? 4 : 2;
    const double win0 = (double)w.a.wrows * w.a.wcols;
    prof_begin(K_WARP, 3.0 * f.rows * f.cols + win0 * (3 * es + 4));
    launch_warp(stream_, lay_.f32, w.src, w.a, g_[0].p, (float*)wgt_[0].p);
    prof_end();
    for (int i = 0; i < L; i++) {
        const Win& d = w.plan.need[i + 1];
        const double nd = (double)(d.x1 - d.x0) * (d.y1 - d.y0);
        prof_begin(K_PYRDOWN_IMG, nd * 4 * 3 * es + nd * 3 * es);
        launch_pyrdown(stream_, lay_.f32 ? 1 : 0, g_[i].p, w.crows >> i, w.ccols >> i, g_[i + 1].p, d.y0, d.y1, d.x0, d.x1);
        prof_end();
        prof_begin(K_PYRDOWN_W, nd * 4 * 4 + nd * 4);
        launch_pyrdown(stream_, 2, wgt_[i].p, w.crows >> i, w.ccols >> i, wgt_[i + 1].p, d.y0, d.y1, d.x0, d.x1);
        prof_end();
    }
    for (int i = 0; i <= L; i++) {
        const double ts = kElePixels >> i, n = (double)(w.bx1 - w.bx0) * (w.by1 - w.by0) * ts * ts;
        prof_begin(K_LAP_SELECT, n * (3 * es + 4 + 4) + (i < L ? n / 4 * 3 * es : 0));
        launch_lap_select(stream_, lay_, i, g_[i].p, i < L ? g_[i + 1].p : nullptr, (const float*)wgt_[i].p,
                          w.crows >> i, w.ccols >> i, w.dtab, w.tx, w.by0, w.by1, w.bx0, w.bx1);
        prof_end();
    }
    return true;
}

// the keyframe is in: its table slot and frame slot retire with the launches, the tiles it touched carry pixels and want a redraw
// (Ischanged, .cpp:553), the cull's weight bounds take this keyframe's
bool FusionMap::retire_frame(const QueuedFrame& f, FrameWork& w, bool fused)
{
    if (!table_pending_[w.ring] && !(fused && opt_.fused == 1)) {
        // this frame's kernels were the last readers of its tile table (fused = 1 retires it in launch_pipeline)
        if (!submitted()) return false;
        table_release_[w.ring] = work_no_;
    }
    if (f.slot >= 0) {
        const hipError_t e = hipEventRecord(slots_[f.slot].consumed, stream_);
        slots_[f.slot].pending = e == hipSuccess;
        release_slot(f);                           // no longer held by the queue: reusable once `consumed` has passed
        HIP_OK(e);
    }
    for (Tile* t : w.touched) { t->fresh = false; t->changed = true; }
    for (Tile* t : w.culled) t->changed = true;
    for (auto& r : w.raise) r.t->wlb[r.q] = std::max(r.t->wlb[r.q], r.w);
    n_rendered_++;
    log_rendered(f);
    return true;
}

#if PF_EXPERIMENTS
// experiments library, PF_CULL_EXACT_STAT=1: level-0 blocks within the pyramid's reach (94 px for five bands) of a cell that is rendered, and
// the same question for the upper levels -- blocks inside the need rectangles against blocks within reach of a rendered cell (printed
// every 100 keyframes).  The accumulators are members: two maps on two threads do not share them.
void FusionMap::cull_exact_stat(const FrameWork& w)
{
    const int L = w.L, tx = w.tx, crows = w.crows, ccols = w.ccols, BHr = level_block_rows(lay_.f32 != 0);
    const Win* C = w.plan.C; const LevelPlan& pl = w.plan;
    const int R0 = 94, nbx = (C[0].x1 - C[0].x0 + 63) / 64, nby = (C[0].y1 - C[0].y0 + BHr - 1) / BHr;
    long cnt = 0;
    for (int gy = 0; gy < nby; gy++)
        for (int gx = 0; gx < nbx; gx++) {
            const int x0 = C[0].x0 + gx * 64 - R0, x1 = C[0].x0 + gx * 64 + 63 + R0, y0 = C[0].y0 + gy * BHr - R0, y1 = C[0].y0 + gy * BHr + BHr - 1 + R0;
            bool need = false;
            for (int qy = std::max(y0, 0) >> 6; qy <= (std::min(y1, crows - 1) >> 6) && !need; qy++)
                for (int qx = std::max(x0, 0) >> 6; qx <= (std::min(x1, ccols - 1) >> 6) && !need; qx++) {
                    const uint64_t e = table_tmp_[(size_t)(qy >> 2) * tx + (qx >> 2)];
                    need = e != 0 && !((e >> (48 + (qy & 3) * 4 + (qx & 3))) & 1);
                }
            cnt += need;
        }
    px_level0_exact_ += (double)cnt * 64 * BHr;
    for (int i = 1; i < L; i++) {
        const int reach = ((3 << (L - i)) - 2) << i, nbxi = (C[i].x1 - C[i].x0 + 63) / 64, nbyi = (C[i].y1 - C[i].y0 + BHr - 1) / BHr;
        for (int gy = 0; gy < nbyi; gy++)
            for (int gx = 0; gx < nbxi; gx++) {
                bool inr = false;
                for (int k = 0; k < pl.nrect[i]; k++) inr = inr || (gx >= pl.rects[i][k].x0 && gx < pl.rects[i][k].x1 && gy >= pl.rects[i][k].y0 && gy < pl.rects[i][k].y1);
                up_rect_[i] += inr;
                const int x0 = ((C[i].x0 + gx * 64) << i) - reach, x1 = ((C[i].x0 + gx * 64 + 64) << i) - 1 + reach;
                const int y0 = ((C[i].y0 + gy * BHr) << i) - reach, y1 = ((C[i].y0 + gy * BHr + BHr) << i) - 1 + reach;
                bool need = false;
                for (int qy = std::max(y0, 0) >> 6; qy <= (std::min(y1, crows - 1) >> 6) && !need; qy++)
                    for (int qx = std::max(x0, 0) >> 6; qx <= (std::min(x1, ccols - 1) >> 6) && !need; qx++) {
                        const uint64_t e = table_tmp_[(size_t)(qy >> 2) * tx + (qx >> 2)];
                        need = e != 0 && !((e >> (48 + (qy & 3) * 4 + (qx & 3))) & 1);
                    }
                up_exact_[i] += need;
            }
    }
    if (++up_n_ % 100 == 0)
        for (int i = 1; i < L; i++) std::fprintf(stderr, "upper level %d: blocks in rectangles %.1f, within reach of a rendered cell %.1f per keyframe\n", i, up_rect_[i] / up_n_, up_exact_[i] / up_n_);
}
#endif

int FusionMap::render_log(long long* out, int cap)
{
    Drained l(*this);
    const int n = (int)std::min<size_t>(render_log_.size(), (size_t)std::max(cap, 0));
    for (int i = 0; i < n; i++) out[i] = render_log_[render_log_.size() - (size_t)n + (size_t)i];
    return (int)render_log_.size();
}

// Retirement without an event per frame (see the header): count the submission, drop a marker now and then.
bool FusionMap::submitted()
{
    work_no_++;
    if (work_no_ % kMarkEvery == 0) {
        HIP_OK(hipEventRecord(mark_ev_[mark_next_], stream_));
        mark_no_[mark_next_] = work_no_;
        mark_next_ = (mark_next_ + 1) % kMarks;
    }
    return true;
}

// block until submission `no` on stream_ has completed
bool FusionMap::wait_for(unsigned long long no)
{
    if (no <= synced_no_) return true;
    int best = -1;
    for (int i = 0; i < kMarks; i++)
        if (mark_no_[i] >= no && (best < 0 || mark_no_[i] < mark_no_[best])) best = i;
    if (best < 0) {                                             // nothing recorded past it yet: mark now
        HIP_OK(hipEventRecord(mark_ev_[mark_next_], stream_));
        mark_no_[mark_next_] = work_no_;
        best = mark_next_;
        mark_next_ = (mark_next_ + 1) % kMarks;
    }
    HIP_OK(hipEventSynchronize(mark_ev_[best]));
    synced_no_ = std::max(synced_no_, mark_no_[best]);
    return true;
}

// One pipelined launch (kernels.hip, k_levels): level 0 of `cur` (if any) and level s of pipe_[s] for every
// pending frame.  A job at level s reads GW_s from the buffer set the previous launch wrote and writes
// GW_{s+1} into this launch's set; stream order between launches is the only synchronisation.
bool FusionMap::launch_pipeline(const PipeFrame* cur, const WarpArgs* wa, const uint8_t* src)
{
    const int L = band_num_;
    const int par = (int)(launch_seq_ & 1);
    DevBuf* out = par ? gw2_ : gw_;
    DevBuf* in  = par ? gw_ : gw2_;
    LevelLaunch jobs[kMaxLevels];
    int n = 0;
    double bytes = 0, bytes_run = 0;
    auto add = [&](const PipeFrame& fr, int i) {
        const bool top = (i + 1 == L);
        LevelLaunch& q = jobs[n++];
        q.level = i; q.rows = fr.crows >> i; q.cols = fr.ccols >> i;
        q.cx0 = fr.C[i].x0; q.cy0 = fr.C[i].y0; q.cx1 = fr.C[i].x1; q.cy1 = fr.C[i].y1;
        q.tiles_x = fr.tx; q.top_select = top; q.write_next = !top; q.from_warp = (i == 0);
        q.gw_in = i == 0 ? nullptr : in[i].p; q.gw_out = top ? nullptr : out[i + 1].p;
        q.table = (const uint64_t*)table_dev_[fr.ring].p;
        q.table_args = i == 0 ? fr.table_args : nullptr; q.table_n = i == 0 ? fr.table_n : 0;
        q.nrect = fr.nrect[i];
        for (int k = 0; k < fr.nrect[i]; k++) q.rect[k] = fr.rect[i][k];
        q.need_bits = i > 0 && fr.need_n[i] > 0 ? fr.need_bits[i] : nullptr; q.need_n = i > 0 ? fr.need_n[i] : 0;
        bytes += fr.bytes[i]; bytes_run += fr.bytes_run[i];
    };
    // level 0 first: the short upper-level blocks come last and fill the tail of the grid
    if (cur) add(*cur, 0);
    static const bool no_upper = exp_env("PF_NO_UPPER") != nullptr;           // experiments library (timing only, wrong tiles): what the upper-level jobs add to a launch
    for (int s = 1; s < L; s++) if (pipe_[s].valid && !no_upper) add(pipe_[s], s);
    if (n) {
        prof_begin(cur ? K_LEVEL0 : K_LEVEL, bytes, stream_, bytes_run);
        launch_levels(stream_, lay_, jobs, n, wa, src);
        prof_end();
        HIP_OK(hipGetLastError());
    }
    // the frame whose last level just ran (this frame itself when L == 1) no longer needs its tile table
    const PipeFrame* done = L >= 2 ? (pipe_[L - 1].valid ? &pipe_[L - 1] : nullptr) : cur;
    if (!submitted()) return false;
    if (done) table_release_[done->ring] = work_no_;
    for (int s = L - 1; s >= 2; s--) pipe_[s] = pipe_[s - 1];
    if (L >= 2) { if (cur) pipe_[1] = *cur; else pipe_[1].valid = false; }
    launch_seq_++;
    return true;
}

// Everything that writes tile slots is ordered before what the caller enqueues on stream_ next (blend, strip pack, tile
// export).  Pipelined path: the pending upper-level launches go onto stream_ itself.  fused = 0/2/3 run pyramid levels on
// streams of their own: wait for those.
bool FusionMap::settle()
{
    if (opt_.fused == 1 || single_band_) return flush_pipeline();
    return sync_all() == hipSuccess;
}

// run the upper levels still pending for the frames fed so far (at most L-1 small launches)
bool FusionMap::flush_pipeline()
{
    if (flushing_) return true;
    flushing_ = true;
    bool ok = true;
    for (;;) {
        bool any = false;
        for (int s = 1; s < kMaxLevels; s++) any = any || pipe_[s].valid;
        if (!any) break;
        if (!launch_pipeline(nullptr, nullptr, nullptr)) { ok = false; break; }
    }
    flushing_ = false;
    return ok;
}

}  // namespace pf
