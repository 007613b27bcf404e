// fusion_map.hpp -- host engine behind the Map2D boundary: the GPU counterpart of
// MultiBandMap2DCPU (Map2DFusion/MultiBandMap2DCPU.h:28-132).
#pragma once
#include "../../include/pifusion.h"
#include "geometry.hpp"
#include "kernels.hpp"
#include "map_support.hpp"
#include "dist_plan.hpp"
#include "frame_plan.hpp"
#include "env.hpp"
#include "image_io.hpp"
#include "jpeg_encode.hpp"
#include "tiff_pyramid.hpp"
#include "png_encode.hpp"
#include "webtiles.hpp"
#include "merge.hpp"
#include "undistort.hpp"
#include "undistort_plan.hpp"
#include <hip/hip_runtime.h>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

namespace pf {

struct FrameSlot {
    uint8_t*   dev = nullptr;
    size_t     cap = 0;
    hipEvent_t consumed = nullptr;    // recorded on the compute stream after the last kernel reading it
    bool       pending = false;       // consumed has been recorded and not yet observed complete
    bool       queued = false;        // sits in the feed queue
};

struct QueuedFrame {
    int    slot;            // index into frame slots, -1 = geometry only
    const uint8_t* ext;     // externally owned device pointer (pf_feed_device) or nullptr
    long   step;
    int    rows, cols, cn;  // cn: 3 = BGR8, 4 = BGRA8
    Pose   pose;            // plane coordinates
    long long seq = -1;     // number of the feed() call that brought it (test hook: render_log)
};

class FusionMap {
public:
    FusionMap(int type, bool thread, const pf_options& opt);
    ~FusionMap();
    bool ok() const { return init_ok_; }

    bool prepare(const double plane[7], const double cam[6], int n, const pf_image* imgs, const double* poses7);
    // `produce` (img->data == nullptr): the frame's pixels are written into HBM by the caller's own work -- it is handed the frame's slot
    // and the stream that work has to be queued on (pf_feed_jpeg: the decoder's upload and kernels); the frame is then queued or rendered
    // exactly as a host frame that feed() uploaded
    typedef std::function<bool(void* dev, hipStream_t stream)> FrameProducer;
    bool feed(const pf_image* img, const double pose[7], bool device_ptr, const FrameProducer* produce = nullptr);
    // pf_feed_raw / pf_feed_raw_device (raw_convert.hpp; DESIGN.md "Raw frames"): feed() of the BGR8 frame the conversion yields, with a
    // producer that gets the planes into HBM (host planes: a blocking copy each, into a scratch slot) and converts them into the frame's slot
    bool feed_raw(const pf_raw_frame* src, const double pose[7], bool device_planes);
    // The input camera (pf_set_input_camera; DESIGN.md "Undistortion"): while one is set, every frame that comes in is a frame of THAT camera
    // (GSLAM parameter vector, n = 6, 7 or 11) and is remapped on the GPU into the map's own pinhole camera before anything else sees it.
    // n = 0 clears it.  It may be set before prepare() and survives prepare(); the table is built and uploaded as soon as both cameras are
    // known.  false (last_error() says why) leaves the map as it was
    bool set_input_camera(const double* in, int n);
    bool input_camera_info(int* rows_in, int* cols_in, long long* uncovered);      // false: none set
    bool has_input_camera() { std::lock_guard<std::mutex> l(mu_); return und_set_; }
    unsigned queue_size();
    long read_back_last_frame(void* out, size_t cap);
    bool sync();
    // save(): the route comes from the name (save_route); save_tiff() (pf_save_tiff): a TIFF under any name, with the tiles' JPEG quality
    // and the flag that forces BigTIFF.  Both are save_file() with the route chosen
    bool save(const char* filename) { return save_file(filename, save_route(filename, single_band_), 95, false); }
    bool save_tiff(const char* filename, int quality, bool force_bigtiff) { return save_file(filename, tiff_route(single_band_), quality, force_bigtiff); }
    // save_tiff() with a transparency mask behind every image (pf_save_tiff_masked): covered = the level-0 weight is not 0
    bool save_tiff_masked(const char* filename, int quality, bool force_bigtiff) { return save_file(filename, tiff_route(single_band_), quality, force_bigtiff, nullptr, true); }
    // the lossless file (pf_save_tiff_lossless): a TIFF under any name with Deflate tiles, masked or not
    bool save_tiff_lossless(const char* filename, bool masked, bool force_bigtiff) { return save_file(filename, tiff_lossless_route(single_band_), 0, force_bigtiff, nullptr, masked); }
    // the mosaic as the PNG of pf_png_encode_bgr under any name (pf_save_png): RGB, or, masked, RGBA with alpha 0 where save() paints the background
    bool save_png(const char* filename, bool masked) { return save_file(filename, png_route(single_band_), 0, false, nullptr, masked); }
    // pf_debug_tiff_counts: tiles, empty tiles and device bytes of the last TIFF this map made on the GPU
    void tiff_counts(size_t* tiles, size_t* empty, size_t* device_bytes) { std::lock_guard<std::mutex> l(mu_); tiff_dev_.last_counts(tiles, empty, device_bytes); }
    // pf_webtiles: what the tiles are made for and where they go
    struct WebTilesJob { const double* gps_origin; int zmin, zmax, quality; bool want_pixels; pf_webtile_sink sink; void* user;
                         double* report; };          // report (may be null): px2ll[6], rows, cols of the mosaic the tiles are made from
    struct ForeignTile { int ix, iy; const void* dev; };          // a tile slot image held outside the store (gathered for save)
    // Where the collapsed mosaic of one save goes.  A value: what the caller asks for, and what save_mosaic() found out on the way
    struct SaveTarget {
        enum Kind { Extent,      // nowhere: rows, cols and the origin tile alone (the first call of pf_save_to_memory)
                    Buffer,      // bgr: the caller's rows * cols * 3 bytes, sized from an earlier Extent call (its second call)
                    Image,       // image: the library's own, sized inside the call from the extent the pixels are made for
                    File,        // a file made on the GPU from the mosaic where it lies in HBM: name, route (a device route), quality, force_bigtiff
                    Tiles };     // Web-Mercator map tiles made on the GPU from the mosaic and its coverage where they lie (webtiles.hpp): web
        Kind kind = Extent;
        const WebTilesJob* web = nullptr;
        uint8_t* bgr = nullptr;
        std::vector<uint8_t>* image = nullptr;
        const char* name = nullptr; SaveRoute route = SaveRoute::HostImage; int quality = 95; bool force_bigtiff = false;
        // the coverage of the same moment, rows * cols bytes, 255 where the level-0 weight is not 0: beside bgr (Buffer; either of
        // the two may be null then), beside image (Image), or as the masks of the file (File, route DeviceTiff)
        uint8_t* mask = nullptr;
        std::vector<uint8_t>* mask_image = nullptr;
        bool masked = false;
        int level = 0;                  // Extent / Buffer without mask only: the mosaic collapsed down to this pyramid level, (256 >> level)^2 pixels a tile
        // results
        bool found = false;             // the map is prepared and holds content: whatever failed after that has said why
        int rows = 0, cols = 0, tx0 = 0, ty0 = 0;
        double transform[16] = {};      // the ModelTransformationTag of a TIFF of this mosaic: pixel -> plane metres
        double plane7[7] = {};          // the plane's pose of the same moment: plane metres -> world
    };
    // ONE pass under mu_: drains, takes the extent, collapses the mosaic and hands it to the target.  foreign: tiles of other ranks
    // that take part without entering the store (dist.cpp)
    bool save_mosaic(SaveTarget& t, const std::vector<ForeignTile>* foreign = nullptr);
    // save_mosaic() into the file: on the GPU, or as pixels through the route's host writer; prints the reference's "Resolution:" line
    bool save_file(const char* filename, SaveRoute route, int quality, bool force_bigtiff, const std::vector<ForeignTile>* foreign = nullptr, bool masked = false);
    // the two-call protocol of pf_save_to_memory: bgr == nullptr reports the extent, bgr takes the pixels of the extent at that moment
    bool save_to_memory(uint8_t* bgr, int* rows, int* cols, int* tx0, int* ty0) { return save_to_memory_mask(bgr, nullptr, rows, cols, tx0, ty0); }
    // ... with the coverage beside the pixels (pf_save_to_memory_mask): both null reports the extent, either may be null after that
    bool save_to_memory_mask(uint8_t* bgr, uint8_t* mask, int* rows, int* cols, int* tx0, int* ty0);
    // ... of the view of pyramid level `level` (pf_save_to_memory_level)
    bool save_to_memory_level(int level, uint8_t* bgr, int* rows, int* cols, int* tx0, int* ty0);
    // pf_webtiles_georef / pf_webtiles (webtiles_plan.hpp, webtiles.hpp): the mosaic of save_to_memory on the globe, and as map tiles.  A
    // multi-band map's tiles are one more device route of save_mosaic(); a single-band map's host mosaic and alpha mask are uploaded
    bool webtiles_georef(const double gps_origin[3], double px2ll[6], int* rows, int* cols);
    bool webtiles(const WebTilesJob& job);
    // pf_render_view* (map_view.cpp; view_plan.hpp, view.hpp; DESIGN.md "Views"): the map after everything fed so far at any pan, zoom,
    // rotation or camera pose, at the size of the caller's window; only the tiles the view depends on are collapsed.  Where it goes:
    struct ViewTarget {
        enum Kind { Host,        // out: host memory (through the output ring)
                    Device,      // out: device memory; queued on `stream` when has_stream, else on the map's stream and complete on return
                    Jpeg };      // the 3-channel view as one JPEG stream in out[0 .. cap), *len its length
        Kind kind = Host;
        uint8_t* out = nullptr; size_t step = 0; int channels = 4;
        hipStream_t stream = nullptr; bool has_stream = false;
        int quality = 95; size_t cap = 0; size_t* len = nullptr;
    };
    bool render_view(const double V[9], int width, int height, int level, const ViewTarget& t, pf_view_info* info);
    // the helpers that only make a V (host code; they read the grid under mu_ without rendering what waits: geometry is in at admission)
    bool view_of_extent(int width, int height, double V[9]);
    bool view_from_pose(const double pose_world7[7], const double* cam6, double V[9]);
    bool view_from_lnglat(const double gps_origin[3], double lng_w, double lat_n, double lng_e, double lat_s, int width, int height, double V[9]);
    void view_timing(bool on) { std::lock_guard<std::mutex> l(mu_); view_timing_ = on; }
    void view_timing_read(double out4[4]) { std::lock_guard<std::mutex> l(mu_); for (int i = 0; i < 4; i++) out4[i] = view_ms_[i]; }

    // seam exchange support (dist.cpp)
    using TileRec = pf::TileRec;        // dist_plan.hpp
    using StripReq = pf::StripReq;
    void list_tiles(std::vector<TileRec>& out);
    bool pack_strips(const std::vector<StripReq>& reqs, void* dev_out);
    bool export_tiles(const std::vector<std::pair<int, int>>& tiles, void* dev_out);
    bool blend_tiles(const std::vector<std::pair<int, int>>& tiles, const void* const* halo9, uint8_t* bgr);
    // frame distribution support (dist.cpp, pf_dist_feed): which ranks hold a tile of this keyframe's canvas (geometry
    // only; applies spreadMap exactly as feed() would, so a later feed of the same pose finds the grid as it left it),
    // a staging slot in HBM for the frame (filled from the host on the root, by the transport elsewhere), and the render
    // of a staged frame
    bool reject_mismatched_frame(const pf_image* desc);      // Map2D::feed's size / type rejection, identical on every rank
    bool frame_needs(const double pose7[7], std::vector<unsigned char>& rank_needs);
    int  stage_frame(const pf_image* desc, bool upload_host, void** dev, size_t* bytes);     // slot index, -1 on failure
    bool feed_staged(int slot, const pf_image* desc, const double pose7[7]);                 // slot < 0: geometry-only feed
    void release_staged(int slot) { std::lock_guard<std::mutex> q(qmu_); if (slot >= 0 && slot < (int)slots_.size()) slots_[slot].queued = false; }
    hipStream_t stream() const { return stream_; }
    int  device() const { return device_; }
    bool use_device() { return set_device(); }
    bool single_band() const { return single_band_; }
    // draw()'s Fuse2Google gate and operands for tile (ix, iy) (MultiBandMap2DCPU.cpp:709-712, :730-735, :744): false when the tile
    // has no pyramid, or lies on the rim of the dense grid while HighQualityShow is on
    bool map_update_inputs(int ix, int iy, double plane7[7], double mn[2], double* ele, int* x, int* y);
    // the cull of render_frame (tiles in which a keyframe cannot win the select): see there, and frame_plan.hpp
    long long culled_tiles() { Drained l(*this); return n_culled_tiles_; }
    void set_cull(bool on) { Drained l(*this); cull_on_ = on; }       // default: on unless PF_CULL=0
    long long culled_cells() { Drained l(*this); return n_culled_cells_; }
    // test hook: the feed() calls (0-based, counted since creation) whose keyframes renderFrame accepted, in render order -- with thread = true
    // and a queue that drops, the only way to tell an oracle which keyframes the map really holds; the newest 65536
    int  render_log(long long* out, int cap);
    double level0_exact_px() const { return px_level0_exact_; }
#if PF_EXPERIMENTS
    // test hook (pf_debug_next_homography): one frame -> canvas matrix per following accepted keyframe, used by frame_canvas() in place of
    // perspective_transform's result and of nothing else -- tests/test_gpu_warp_ties.py chooses the warp's coordinates with it
    void debug_next_homography(const double M0[9]) { std::lock_guard<std::mutex> l(mu_); next_M0_.emplace_back(); std::memcpy(next_M0_.back().m, M0, sizeof(double) * 9); }
    // test hooks (pf_debug_tile_store / pf_debug_fail_workspace): allocation failures on request -- tests/test_gpu_alloc_failure.py.  Neither
    // renders what waits: a test arms them between two feeds without emptying the lookahead window
    void debug_tile_store(int slab_slots, int fail_from, int fail_count) { std::lock_guard<std::mutex> l(mu_); store_.debug_limits(slab_slots, fail_from, fail_count); }
    void debug_fail_workspace(int n) { std::lock_guard<std::mutex> l(mu_); dbg_fail_workspace_ = n; }
#endif
    bool high_quality() const { return opt_.high_quality_show != 0 && !single_band_; }

    int  num_levels() const { return band_num_ + 1; }
    int  pyramid_type() const { return single_band_ ? PF_8UC4 : (lay_.f32 ? PF_32FC3 : PF_16SC3); }
    bool grid(int dims[4], double geo[6]);
    int  tile_count();
    int  tile_coords(int* xy, int cap);
    bool get_tile_level(int ix, int iy, int level, void* lap, float* w);
    bool get_tile_bgra(int ix, int iy, uint8_t* bgra);
    bool blend_tile(int ix, int iy, void* raw, uint8_t* bgr, const void* const* halo);
    int  blend_changed(int* xy, uint8_t* bgr, int cap, int level = 0);
    bool blend_list(const std::vector<std::pair<int, int>>& tiles, uint8_t* bgr);      // pf_blend_tiles: Ischanged left alone
    // views of pyramid level `level` (collapse_level.hip): (256 >> level)^2 pixels a tile, bgr and / or raw (either may be null)
    bool blend_list_level(const std::vector<std::pair<int, int>>& tiles, int level, uint8_t* bgr, void* raw);
    bool level_ok(const char* who, int level);      // false, with the reason in last_error(): no such level / no pyramid / a sharded map above level 0
    // pf_blend_tiles_jpeg: the same tiles as n JPEG streams back to back, offsets[0..n]; the blended pixels stay in HBM
    struct TileJpeg { int quality; uint8_t* out; size_t cap; size_t* offsets; size_t used = 0; };
    bool blend_list_jpeg(const std::vector<std::pair<int, int>>& tiles, int quality, uint8_t* out, size_t cap, size_t* offsets);
    size_t halo_bytes_for(int dx, int dy) const { return halo_bytes(lay_, dx, dy); }
    bool halo_pack(int ix, int iy, int dx, int dy, void* dev_out);
    size_t tile_bytes() const { return lay_.slot_bytes; }
    bool tile_export(int ix, int iy, void* dev_out);
    bool tile_import(int ix, int iy, const void* dev_in);
    // Map merge (merge.hpp): src's tiles selected into this map's, by stable tile coordinate -- the map that was fed
    // this map's keyframes and then src's, bit for bit.  Both maps prepared alike on one device, neither sharded; src is not modified.
    // Refusals (false, last_error() says why) touch nothing.
    bool merge_from(FusionMap& src);
    // ... from n slot images the caller holds in this device's memory (what tile_export writes; 16-byte aligned), at stable coordinates
    // xy[2n].  wlb16: 16 cull bounds per tile, or null when nothing is known of them (not finite: -1)
    bool merge_tiles(int n, const int* xy, const void* const* dev_slots, const float* wlb16);
    bool tile_bounds(int ix, int iy, float wlb16[16]);      // the tile's cull bounds, to travel with tile_export's image
    // The state file (state_file.hpp): save_state writes this map's whole state; load_state is "prepare from the file" (the map's own
    // options must be the file's); merge_state merges the file's tiles into this prepared, compatible map as merge_from would
    bool save_state(const char* path);
    bool load_state(const char* path);
    bool merge_state(const char* path);
    // the most recent merge: pairs, pairs whose dst was fresh, ms between HIP events around its launches, pixel-levels src won (-1: not
    // counted), slot bytes, 0.  count_stores >= 0 switches the counting (one atomic per thread: measurement only) for the merges to come
    void merge_stats(int count_stores, double out[6]);

    void profile_enable(int mode);
    int  profile_read(int cap, const char** names, double* ms, long long* launches, double* bytes, double* bytes_run = nullptr);
    void profile_reset();
    void stats(long long* rendered, long long* rejected, long long* dropped, long long* failed = nullptr);
    void render_stats(double out[4]);
    int  timer_read(int cap, const char** names, long long* calls, double* mean_s, double* min_s, double* max_s);
    void timer_reset();
    struct Section {            // scope guard: enter on construction, leave on destruction
        FusionMap* m; int id; double t0;
        Section(FusionMap* m_, int id_);
        ~Section();
    };
    bool reserve_tiles(long long n_tiles);
    const pf_options& options() const { return opt_; }

private:
    bool render_frame(const QueuedFrame& f);                       // .cpp:311-558
    bool spread_map(double xmin, double ymin, double xmax, double ymax);   // .cpp:561-604
    void spread_tiles(const Win& r);                               // ... its second half: the grid grown to hold dense tile range r
    // footprint -> bounding box -> spreadMap when it leaves the grid -> tile range r (dense index); box: xmin, ymin, xmax, ymax
    bool canvas_range(const double pts[8], Win& r);
    void tile_range(double xmin, double ymin, double xmax, double ymax, Win& r) const;
    // (while an input camera is set, the frames that come in have ITS size)
    bool frame_mismatch(int type, int cols, int rows) const
    {
        if (und_set_) return (type != PF_8UC3 && type != PF_8UC4) || cols != und_cam_.w || rows != und_cam_.h;
        return (type != PF_8UC3 && type != PF_8UC4) || cols != cam_.w || rows != cam_.h;
    }
    void worker();                                                 // .cpp:619-635
    int  acquire_slot(size_t bytes);
    bool upload(const pf_image* img, int slot);
    // The one producer of undistorted frames: the raw frame (host pixels, a caller's device pointer, or what `produce` writes) goes into a
    // scratch slot -- a device pointer is read where it lies -- and k_undistort writes the frame's own slot on stream_.  Both slots carry a
    // `consumed` event behind the kernel, like any frame slot.  Returns the frame's slot (packed BGR8 of the map's camera), -1 on failure
    int  undistort_frame(const pf_image* img, bool device_ptr, const FrameProducer* produce);
    bool produce_raw(const pf_raw_frame& src, bool device_planes, uint8_t* dst, hipStream_t st);          // called with mu_ held, by feed()
    bool build_undistort_table(const undistort::InCamera& in, const Camera& out, DevBuf& buf, long long* uncovered);
    bool blend_batch(const std::vector<std::pair<int,int>>& tiles, const void* const* halo9, void* raw_host, uint8_t* bgr_host, TileJpeg* jpeg = nullptr, int level = 0);
    // the kernel-event profiler (KernelProfiler, map_support.hpp) around a launch; st: the stream it goes to, stream_ when null
    void prof_begin(int id, double bytes, hipStream_t st = nullptr, double bytes_run = -1) { prof_.begin(id, bytes, st ? st : stream_, bytes_run); }
    bool prof_would(int id) const { return prof_.would(id); }
    hipError_t sync_all();
    void prof_end() { if (prof_.end()) { (void)sync_all(); prof_.harvest(); } }
    bool set_device();
    // THE DRAIN RULE: every reader of the map's state -- tiles, flags, counters -- takes mu_ and renders the keyframes that wait in the
    // lookahead window before it looks (drain()).  That is what makes the lookahead exact (PendingFrame, below): what a caller can observe
    // after feed() k is the map after keyframes 1 .. k.  A reader holds one of these; a site that takes mu_ and must NOT render what waits
    // (the debug hooks, profile_enable, the input camera) holds a plain lock_guard and says so.  A drain that fails has counted its
    // keyframes (keyframe_lost()); the next sync() reports them
    struct Drained {
        std::lock_guard<std::mutex> l;
        explicit Drained(FusionMap& m) : l(m.mu_) { (void)m.drain(); }
    };

    pf_options opt_;
    int        band_num_ = 5;
    TileLayout lay_{};
    bool       thread_ = false, init_ok_ = false;
    bool       single_band_ = false;      // Map2DCPU semantics (TypeCPU / TypeGPU), one BGRA tile per cell
    DevBuf     w8_; int w8_rows_ = 0, w8_cols_ = 0;   // its weight byte plane
    DevBuf     wmap_; int wmap_rows_ = 0, wmap_cols_ = 0;   // multi-band: fp32 weight plane (weightImage)
    int        device_ = 0;
    hipStream_t stream_ = nullptr;

    // prepared state, guarded by mu_
    std::mutex mu_;
    bool   valid_ = false;
    Pose   plane_{}, plane_inv_{};
    bool cull_on_ = !(std::getenv("PF_CULL") && std::atoi(std::getenv("PF_CULL")) == 0);
    long long n_culled_tiles_ = 0;              // tiles left out of launches by the cull (diagnostics)
    long long n_culled_cells_ = 0;              // 64 x 64 cells of rendered tiles switched off by it
    // Margins of the cull's bounds (frame_plan.hpp, CullMargins).  PF_CULL_MARGIN_PX / PF_CULL_MARGIN_W (experiments library) override them for
    // the sensitivity runs of tools/cull_soak.py (profiles/r05_cull_margins.md: mismatches against the oracle per setting -- the safety
    // factor, measured); defaults 2 px, 1e-5.  PF_CULL_SUB (experiments library): cells per tile edge, 2 = quadrants
    CullMargins cull_margins_{ exp_env_double("PF_CULL_MARGIN_PX", 2.0), exp_env_double("PF_CULL_MARGIN_W", 1e-5), exp_env_int("PF_CULL_SUB", 4) == 2 ? 2 : 4 };
    Camera cam_{};
    double ele_size_ = 0, ele_size_inv_ = 0, length_pixel_ = 0, length_pixel_inv_ = 0;
    double min_[3]{}, max_[3]{};
    double min0_[3]{};                          // min_ as prepare computed it: the origin of the stable tile coordinates (merge: same frame <=> same min0_, ele_size_)
    int    w_ = 0, h_ = 0, off_x_ = 0, off_y_ = 0;
    TileStore store_;

    // per-frame workspace (grow-only)
    DevBuf g_[kMaxLevels], wgt_[kMaxLevels], gw_[kMaxLevels], gw2_[kMaxLevels];
    hipStream_t lvl_stream_[kMaxLevels]{};          // fused pipeline: one stream per level ([0] aliases stream_)
    static constexpr int kTableRing = 64;           // tile tables in flight (see retire())
    static constexpr int kLvlRing = 16;
    hipEvent_t  lvl_ev_[kMaxLevels][kLvlRing]{};    // fused = 2/3: level i of the frame in ring slot k has run
    static constexpr int kUpperStreams = 1;         // streams shared by pyramid levels >= 1
    // Tile tables live in device memory (table_dev_, a ring of kTableRing per-frame tables).  How a frame's table gets
    // there: inside the kernel arguments of the launch that carries the frame's level 0, which stores it to the ring slot
    // itself (pipelined path, tables of at most kArgTable entries: nothing sits in the stream between two launches and
    // no host memory is read in place); otherwise staged in pinned host memory and copied in the stream.
    uint64_t*  table_host_[kTableRing]{};           // pinned staging of the copy path
    bool       table_in_args_ = true;               // PF_TABLE_COPY=1 forces the copy path (A/B, tests)
    DevBuf     table_dev_[kTableRing];
    std::vector<uint64_t> table_tmp_;               // a frame's entries while they are being built
    size_t     table_cap_ = 0;
    hipEvent_t table_ev_[kTableRing]{};             // fused = 2/3: last reader of the ring slot done (own stream)
    bool       table_pending_[kTableRing]{};
    // Everything else retires on stream_, and an event record between two dependent launches costs ~18 us of
    // stream time on this stack: instead of one event per frame, a ring slot remembers the number of the launch that
    // reads it last (work_no_ counts submissions on stream_), a marker event is recorded every kMarkEvery
    // submissions, and a slot is reused after waiting for a marker at or past its number.
    static constexpr int kMarkEvery = 32, kMarks = 4;           // kTableRing - kMaxLevels >= kMarkEvery
    unsigned long long work_no_ = 0, synced_no_ = 0;
    unsigned long long table_release_[kTableRing]{};
    hipEvent_t mark_ev_[kMarks]{};
    unsigned long long mark_no_[kMarks]{};
    int  mark_next_ = 0;
    bool submitted();                                           // call once per submission on stream_
    bool wait_for(unsigned long long no);
    unsigned long long frame_seq_ = 0;

    // pipelined level launches (opt_.fused == 1): pipe_[s] is the frame whose level s runs in the next launch
    struct PipeFrame { bool valid = false; int ring = 0, tx = 0, crows = 0, ccols = 0; Win C[kMaxLevels]; double bytes[kMaxLevels], bytes_run[kMaxLevels];
                       int nrect[kMaxLevels]; BlockRect rect[kMaxLevels][kMaxRects];        // LevelLaunch::rect of each level
                       uint32_t need_bits[kMaxLevels][kNeedWords]; int need_n[kMaxLevels] = {};    // LevelLaunch::need_bits of the upper levels (need_n 0: none)
                       const uint64_t* table_args = nullptr; int table_n = 0; };            // level 0 only, valid during render_frame
    PipeFrame pipe_[kMaxLevels];
    // One keyframe on its way through render_frame (MultiBandMap2DCPU::renderFrame, .cpp:311-558): what each stage leaves for the next.
    // Kept in the map between keyframes so that its vectors keep their capacity (render_frame runs on one thread at a time).
    struct FrameWork {
        // frame_canvas(): footprint, tile range, homography
        double pts[8]; int xminInt, yminInt, xmaxInt, ymaxInt;
        int tx, ty, L, crows, ccols; double M0[9], Minv[9];
        const uint8_t* src;
        // build_tile_table(): the cull (lat: the keyframe's lattice), the owned tiles and their boxes (tiles; level-0 pixels), the hash cells of the need rectangles
        bool sharded, cull, culled_any; Lattice* lat;
        bool pre_raised;                                          // the keyframe's bounds entered wlb when it was admitted (lookahead): not worked out again
        Tile* const* tiles_known;                                 // ... and its canvas' tiles are known from then (nullptr: look them up)
        struct Raise { Tile* t; int q; float w; };                // (cell, wmin of this keyframe): applied once the frame is in
        std::vector<Raise> raise; std::vector<Tile*> culled, touched;
        CellList cells;
        int bx0, bx1, by0, by1, owned, owned_all;
        Win pb;
        // where each level is needed and which blocks run (frame_plan.hpp)
        LevelPlan plan;
        // place_table() / warp_args()
        int ring; bool table_args; const uint64_t* dtab;
        WarpArgs a;
        void reset() {
            raise.clear(); culled.clear(); touched.clear();
            culled_any = cells.overflow = false; cells.n = 0; owned = owned_all = 0; plan.reset();
            src = nullptr; ring = 0; table_args = false; dtab = nullptr; sharded = cull = pre_raised = false; tiles_known = nullptr; lat = nullptr;
        }
    };
    FrameWork fw_;
    // Keyframes that are in (geometry done, grid advanced, tiles created, their weight bounds raised) but not rendered yet: the LOOKAHEAD of the
    // cull (round 6).  The max-weight select is order independent -- a pixel-level ends with the largest weight, the newest keyframe among equals
    // (.cpp:521, :542 `>=`; a fresh tile's unconditional copy is the same select against weight 0) -- so a keyframe may be left out of a cell not
    // only where an EARLIER keyframe's weights bound it from above (rounds 4-5) but also where a LATER one's do, provided that later keyframe is
    // certain to be rendered before anybody looks: every reader of the map's state drains this queue first (drain()), so what a caller can
    // observe after feed() k is exactly the map after keyframes 1..k.  opt_.lookahead keyframes wait here (0: render inside feed() as before).
    struct PendingFrame {
        QueuedFrame f;
        double pts[8]; int sx0, sy0, tx, ty;        // canvas origin in STABLE tile coordinates (dense index + accumulated spreadMap offset)
        double M0[9], Minv[9];
        bool cull;
        Lattice lat;                                // the cull's lattice of this keyframe (cull only)
        bool pre_raised = false;                    // lookahead: the keyframe's lower bounds entered the tiles' wlb when it was admitted
        std::vector<Tile*> tiles;                   // ... and the canvas' tiles were looked up / created then (row-major; nullptr: another shard's)
    };
    std::deque<PendingFrame> pending_;
    // The window FILLS at two keyframes per three feeds after it was last emptied (a reader, pf_sync): the first keyframe behind a sync is
    // rendered at once and every third one after it (an admission costs the host ~25 us, a launch keeps the GPU busy for ~90), so the GPU
    // does not idle while `lookahead` keyframes gather, and a short burst between two readers is not held up
    unsigned since_drain_ = 0;
    std::vector<Lattice> lat_pool_;                 // buffers of rendered keyframes' lattices, reused
    std::vector<std::vector<Tile*>> tiles_pool_;
    bool lookahead_ok() const { return opt_.lookahead > 0 && (single_band_ || (opt_.fused == 1 && band_num_ >= 1)) && cull_on_; }     // wherever the cull runs
    bool render_front();                            // renders pending_.front() and removes it; a failure is counted (keyframe_lost)
    bool render_front_stages();                     // ... its stages 4 onwards
    bool drain();                                   // ... all of them; mu_ held (the drain rule: Drained, above)
    void release_slot(const QueuedFrame& f);
    bool pre_raise(FrameWork& w, std::vector<Tile*>& tiles);
    // A keyframe that was accepted (its geometry is in, the grid has advanced) and is not in the map, because an allocation or a launch
    // failed: counted, and the message kept for the next sync() -- whichever thread and whichever call met the failure (mu_ held)
    void keyframe_lost() { n_failed_++; fail_pending_ = true; fail_msg_ = last_error(); }
    long long n_failed_ = 0;
    bool fail_pending_ = false;
    std::string fail_msg_;
#if PF_EXPERIMENTS
    int dbg_fail_workspace_ = 0;                    // debug_fail_workspace(): reserve_frame_workspace calls that still have to fail
#endif
    int  frame_canvas(const QueuedFrame& f, FrameWork& w);
    bool build_tile_table(const QueuedFrame& f, FrameWork& w);
    bool reserve_frame_workspace(FrameWork& w);
    bool place_table(FrameWork& w);
    void warp_args(const QueuedFrame& f, FrameWork& w);
    void plan_fused_levels(FrameWork& w);
    bool launch_single_band(const QueuedFrame& f, FrameWork& w);
    bool launch_fused_pipeline(const QueuedFrame& f, FrameWork& w);
    bool launch_level_streams(const QueuedFrame& f, FrameWork& w);
    bool launch_per_op(const QueuedFrame& f, FrameWork& w);
    bool retire_frame(const QueuedFrame& f, FrameWork& w, bool fused);
    void log_rendered(const QueuedFrame& f);
    unsigned long long launch_seq_ = 0;             // parity selects the GW buffer set a launch writes
    bool flushing_ = false;
    bool launch_pipeline(const PipeFrame* cur, const WarpArgs* wa, const uint8_t* src);
    bool flush_pipeline();
    bool settle();

    // blend / save scratch (blend_lv_: the per-level form of the experiments library only)
    DevBuf blend_lv_[kMaxLevels], blend_src_, blend_out_raw_, blend_out_bgr_, mosaic_table_, strip_desc_;
    DevBuf cover_plane_, cover_bytes_;          // pf_save_to_memory_mask: the mosaic's coverage as a bit plane (coverage.hip), and as bytes
    TiffDevice  tiff_dev_;      // save("x.tif"): level buffers and flags of its own, tiles through jpeg_enc_
    DeflateEncoder deflate_enc_;   // save_tiff_lossless(): the tiles of tiff_dev_'s levels on stream_, buffers of its own
    PngEncoder  png_enc_;       // save_png(): reads blend_out_bgr_ (and cover_bytes_) on stream_, buffers of its own
    JpegEncoder jpeg_enc_;      // save("x.jpg"), pf_blend_tiles_jpeg: reads blend_out_bgr_ on stream_, buffers of its own
    OutRing     out_ring_;      // results on their way to the host
    bool export_webtiles(const SaveTarget& t, const WebTilesJob& job);                        // blend_out_bgr_ + cover_bytes_ of extent t -> the job's map tiles
    bool save_to_caller(SaveTarget& t, int* rows, int* cols, int* tx0, int* ty0);             // save_mosaic() + the extent handed back
#if PF_EXPERIMENTS
    bool blend_batch_per_level(const std::vector<std::pair<int,int>>& tiles, const void* const* halo9, void* raw_host, uint8_t* bgr_host);
#endif

    // map merge / state file
    struct MergeItem { int ix, iy; const void* src; const float* wlb; };      // wlb: 16 bounds of the src tile, or null
    bool merge_items(const std::vector<MergeItem>& items);         // mu_ held, drained: tiles created first, one table, launches in batches, flags and bounds
    bool merge_compatible(const char* who, bool single, int pyr, int bands, int weight_type, const double plane7[7], const double cam6[6],
                          const double min0[3], double ele_size, double length_pixel);
    void grow_to(int sx0, int sy0, int sx1, int sy1);              // the grid grown to hold stable tile range [sx0, sx1) x [sy0, sy1)
    bool merge_records(std::FILE* f, const void* header, const void* heads);      // state_file.hpp's StateHeader / vector<TileHead>
    void wait_worker_idle();
    DevBuf merge_table_, merge_stage_, merge_won_;
    hipEvent_t merge_ev_[2]{};
    bool   merge_count_ = false;
    double last_merge_[6] = { 0, 0, 0, -1, 0, 0 };

    // views (map_view.cpp): the sub-table of the rectangle's tile pointers, the collapsed rectangle (BGR8), its coverage (a byte a
    // pixel) and the view itself on its way to the host or the encoder
    DevBuf view_table_, view_bgr_, view_cover_, view_out_;
    hipEvent_t view_ev_[6]{};                   // [0..3] timing hook (pf_debug_view_timing): around the collapse, the coverage pass and the view kernel; [4], [5]: order against a caller's stream
    bool   view_timing_ = false;
    double view_ms_[4] = { 0, 0, 0, 0 };        // ... their milliseconds in the most recent view, and the tiles it collapsed

    // input camera (guarded by mu_): und_table_ holds the remap table for (und_cam_, cam_) whenever und_set_ && valid_
    bool und_set_ = false;
    undistort::InCamera und_cam_{};
    DevBuf und_table_;
    long long und_uncovered_ = 0;

    // frame staging + feed queue
    std::vector<FrameSlot> slots_;
    int    last_slot_ = -1; size_t last_bytes_ = 0;       // most recent upload (read_back_last_frame)
    std::mutex qmu_;
    std::condition_variable qcv_, idle_cv_;
    std::deque<QueuedFrame> queue_;
    bool worker_busy_ = false, stop_ = false;
    std::thread worker_;

    // profile
    KernelProfiler prof_;
    SectionRec sections_[T_COUNT];
    std::mutex timer_mu_;
    long long n_rendered_ = 0, n_rejected_ = 0, n_dropped_ = 0, n_with_pixels_ = 0;
    long long feed_seq_ = 0; std::vector<long long> render_log_;
    double px_level0_exact_ = 0;                    // experiments library, PF_CULL_EXACT_STAT (statistics of the cull, cull_exact_stat())
#if PF_EXPERIMENTS
    struct Mat9 { double m[9]; };
    std::deque<Mat9> next_M0_;                      // debug_next_homography(): consumed by frame_canvas(), oldest first
    double up_rect_[kMaxLevels] = {}, up_exact_[kMaxLevels] = {}; long up_n_ = 0;
    void cull_exact_stat(const FrameWork& w);
#endif
    double px_level0_ = 0, px_owned_ = 0;           // level-0 pixels computed (with halo) / tile pixels owned, over the frames rendered
};

}  // namespace pf
