// fusion_map.cpp -- host engine: prepare / feed / renderFrame / blend / save on
// the GPU, following the control flow of Map2DFusion/MultiBandMap2DCPU.cpp.
#include "fusion_map.hpp"
#include "webtiles_plan.hpp"
#include "env.hpp"
#include "warp_index.hpp"
#include "coverage.hpp"
#include "state_file.hpp"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <dlfcn.h>

namespace pf {

static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; std::fprintf(stderr, "pifusion: %s\n", msg.c_str()); }
const char* last_error() { return g_err.c_str(); }

#define HIP_OK(expr)                                                                       \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess) {                                                            \
            set_error(std::string(#expr) + ": " + hipGetErrorString(e_));                  \
            return false;                                                                  \
        }                                                                                  \
    } while (0)

static inline int floordiv(int a, int b) { int q = a / b; if ((a % b != 0) && ((a < 0) != (b < 0))) q--; return q; }

int tile_owner(int shard_count, int shard_block, int ix, int iy)
{
    if (shard_count <= 1) return 0;
    const int b = shard_block > 0 ? shard_block : 8;
    // PF_SHARD_OWNER_CYCLIC=1 (experiments library; evaluation only, tools/predict_scaling.py --owner cyclic; every rank must set it alike): SURVEY 8e's other
    // candidate, a 2-D block-cyclic owner -- cells dealt over a px x py grid of ranks (px * py = shard_count, px the larger factor), so that
    // neighbouring cells never share a rank and any px x py window of cells holds every rank once
    static const bool cyclic = exp_env_int("PF_SHARD_OWNER_CYCLIC", 0) != 0;     // experiments library only
    if (cyclic) {
        int py = 1;
        for (int d = 1; d * d <= shard_count; d++) if (shard_count % d == 0) py = d;
        const int px = shard_count / py, cxs = floordiv(ix, b), cys = floordiv(iy, b);
        return ((cxs % px) + px) % px + px * (((cys % py) + py) % py);
    }
    const uint32_t cx = (uint32_t)floordiv(ix, b), cy = (uint32_t)floordiv(iy, b);
    const uint32_t h = (cx * 73856093u) ^ (cy * 19349663u);
    return (int)(h % (uint32_t)shard_count);
}

// --------------------------------------------------------------- sections
const char* section_name(int id)
{
    static const char* n[T_COUNT] = { "Map2D::feed", "MultiBandMap2DCPU::renderFrame", "MultiBandMap2DCPU::Apply",
                                      "MultiBandMap2DCPU::spreadMap", "MultiBandMap2DCPU::updateTexture", "MultiBandMap2DCPU::save" };
    return (id >= 0 && id < T_COUNT) ? n[id] : "?";
}

// roctx ranges (libroctx64 is looked up at run time, only when PF_ROCTX is set)
namespace {
struct Roctx { bool tried = false; int (*push)(const char*) = nullptr; int (*pop)() = nullptr; };
Roctx g_roctx;
void roctx_load()
{
    g_roctx.tried = true;
    if (!std::getenv("PF_ROCTX")) return;
    void* h = dlopen("libroctx64.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("/opt/rocm/lib/libroctx64.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("librocprofiler-sdk-roctx.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) { std::fprintf(stderr, "pifusion: PF_ROCTX set but no roctx library found\n"); return; }
    *(void**)&g_roctx.push = dlsym(h, "roctxRangePushA");
    *(void**)&g_roctx.pop = dlsym(h, "roctxRangePop");
}
}  // namespace
void roctx_push(const char* name) { if (!g_roctx.tried) roctx_load(); if (g_roctx.push) g_roctx.push(name); }
void roctx_pop() { if (g_roctx.pop) g_roctx.pop(); }

static inline double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

FusionMap::Section::Section(FusionMap* m_, int id_) : m(m_), id(id_), t0(now_s()) { roctx_push(section_name(id)); }
FusionMap::Section::~Section()
{
    roctx_pop();
    const double dt = now_s() - t0;
    std::lock_guard<std::mutex> l(m->timer_mu_);
    SectionRec& r = m->sections_[id];
    if (!r.n_calls || dt < r.min_t) r.min_t = dt;
    if (dt > r.max_t) r.max_t = dt;
    r.total_t += dt; r.n_calls++;
}

int FusionMap::timer_read(int cap, const char** names, long long* calls, double* mean_s, double* min_s, double* max_s)
{
    std::lock_guard<std::mutex> l(timer_mu_);
    int n = 0;
    for (int i = 0; i < T_COUNT && n < cap; i++, n++) {
        const SectionRec& r = sections_[i];
        if (names) names[n] = section_name(i);
        if (calls) calls[n] = r.n_calls;
        if (mean_s) mean_s[n] = r.n_calls ? r.total_t / r.n_calls : 0;
        if (min_s) min_s[n] = r.min_t;
        if (max_s) max_s[n] = r.max_t;
    }
    return n;
}

void FusionMap::timer_reset() { std::lock_guard<std::mutex> l(timer_mu_); for (auto& r : sections_) r = SectionRec(); }

// ------------------------------------------------------------------ store
Tile* TileStore::find(int ix, int iy)
{
    auto it = map_.find(key(ix, iy));
    return it == map_.end() ? nullptr : &it->second;
}

bool TileStore::add_chunk(size_t slots)
{
    void* p = nullptr;
    size_t bytes = slots * slot_bytes_;
#if PF_EXPERIMENTS
    if (dbg_count_ > 0) { const long no = dbg_no_++; if (no >= dbg_from_ && no < dbg_from_ + dbg_count_) bytes = (size_t)1 << 60; }      // debug_limits()
#endif
    // (a refused hipMalloc stays behind as the thread's last HIP error: taken off here, or the next launch check reports it as its own)
    if (hipMalloc(&p, bytes) != hipSuccess) { (void)hipGetLastError(); set_error("tile store: hipMalloc failed"); return false; }
    chunks_.push_back({ (char*)p, slots });
    return true;
}

size_t TileStore::slab_slots() const
{
#if PF_EXPERIMENTS
    if (dbg_slab_) return dbg_slab_;
#endif
    return std::max<size_t>(16, (256u << 20) / slot_bytes_);
}

Tile* TileStore::get_or_create(int ix, int iy)
{
    auto it = map_.find(key(ix, iy));
    if (it != map_.end()) return &it->second;
    if (chunks_.empty()) { if (!add_chunk(slab_slots())) return nullptr; cur_ = 0; next_in_chunk_ = 0; }
    if (next_in_chunk_ == chunks_[cur_].slots) {
        if (cur_ + 1 == chunks_.size() && !add_chunk(slab_slots())) return nullptr;
        cur_++; next_in_chunk_ = 0;
    }
    Tile t;
    t.base = chunks_[cur_].p + next_in_chunk_++ * slot_bytes_;
    return &map_.emplace(key(ix, iy), t).first->second;
}

// pre-size the store (std::vector::reserve for HBM): one slab for what the slabs at hand cannot hold
bool TileStore::reserve(size_t n_tiles, std::vector<std::pair<char*, size_t>>* fresh)
{
    size_t have = 0;
    for (size_t i = cur_; i < chunks_.size(); i++) have += chunks_[i].slots - (i == cur_ ? next_in_chunk_ : 0);
    if (have >= n_tiles) return true;
    const size_t want = std::max<size_t>(n_tiles - have, 16);
    if (!add_chunk(want)) return false;
    if (fresh) fresh->push_back({ chunks_.back().p, want * slot_bytes_ });
    return true;
}

void TileStore::clear()
{
    for (auto& c : chunks_) (void)hipFree(c.p);
    chunks_.clear(); map_.clear(); next_in_chunk_ = cur_ = 0;
}

bool DevBuf::reserve(size_t bytes)
{
    if (bytes <= cap) return true;
    release();
    const size_t want = bytes + bytes / 4;
    if (hipMalloc(&p, want) != hipSuccess) { (void)hipGetLastError(); p = nullptr; set_error("hipMalloc failed"); return false; }
    cap = want;
    return true;
}
void DevBuf::release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }

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
    prof_harvest();
    for (auto e : ev_pool_) (void)hipEventDestroy(e);
    for (int i = 0; i < kMaxLevels; i++) {
        bool shared = lvl_stream_[i] == stream_;
        for (int k = 1; k < i; k++) shared = shared || lvl_stream_[k] == lvl_stream_[i];
        if (i > 0 && lvl_stream_[i] && !shared) (void)hipStreamDestroy(lvl_stream_[i]);
        for (int k = 0; k < kLvlRing; k++) if (lvl_ev_[i][k]) (void)hipEventDestroy(lvl_ev_[i][k]);
        gw_[i].release(); gw2_[i].release();
    }
    for (auto& s : slots_) { if (s.dev) (void)hipFree(s.dev); if (s.consumed) (void)hipEventDestroy(s.consumed); }
    for (int i = 0; i < kTableRing; i++) {
        if (table_host_[i]) (void)hipHostFree(table_host_[i]);
        table_dev_[i].release();
        if (table_ev_[i]) (void)hipEventDestroy(table_ev_[i]);
        if (i < kMarks && mark_ev_[i]) (void)hipEventDestroy(mark_ev_[i]);
    }
    for (int i = 0; i < kMaxLevels; i++) { g_[i].release(); wgt_[i].release(); blend_lv_[i].release(); }
    for (int i = 0; i < 2; i++) { if (out_pin_[i]) (void)hipHostFree(out_pin_[i]); if (out_copied_[i]) (void)hipEventDestroy(out_copied_[i]); }
    if (out_ready_) (void)hipEventDestroy(out_ready_);
    if (copy_stream_) (void)hipStreamDestroy(copy_stream_);
    blend_src_.release(); blend_out_raw_.release(); blend_out_bgr_.release(); mosaic_table_.release(); w8_.release(); wmap_.release();
    cover_plane_.release(); cover_bytes_.release();
    merge_table_.release(); merge_stage_.release(); merge_won_.release(); und_table_.release();
    for (auto e : merge_ev_) if (e) (void)hipEventDestroy(e);
    jpeg_enc_.release(); tiff_dev_.release();
    store_.clear();
    (void)hipStreamDestroy(stream_);
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

// ---------------------------------------------------------------- profile
void FusionMap::profile_enable(int mode) { std::lock_guard<std::mutex> l(mu_); prof_mode_ = mode; }

bool FusionMap::prof_would(int id) const
{
    const int what = prof_mode_ & 0xff, every = prof_mode_ >> 8;
    return (what == 1 || what == 2 + id) && (every <= 1 || prof_tick_[id] % every == 0);
}

void FusionMap::prof_begin(int id, double bytes, hipStream_t st, double bytes_run)
{
    prof_stream_ = st ? st : stream_;
    const int what = prof_mode_ & 0xff, every = prof_mode_ >> 8;
    prof_on_ = what == 1 || what == 2 + id;                  // mode 2+k: only kernel k
    // event pairs are not free (each is a marker packet between two launches): optionally time every n-th launch only
    if (prof_on_ && every > 1) prof_on_ = (prof_tick_[id]++ % every) == 0;
    if (!prof_on_) return;
    auto get = [&]() { hipEvent_t e; if (!ev_pool_.empty()) { e = ev_pool_.back(); ev_pool_.pop_back(); } else (void)hipEventCreate(&e); return e; };
    prof_cur_ = { id, get(), get(), bytes, bytes_run < 0 ? bytes : bytes_run };
    (void)hipEventRecord(prof_cur_.a, prof_stream_);
}

void FusionMap::prof_end()
{
    if (!prof_on_) return;
    (void)hipEventRecord(prof_cur_.b, prof_stream_);
    prof_pending_.push_back(prof_cur_);
    if (prof_pending_.size() > 4096) { (void)sync_all(); prof_harvest(); }
}

void FusionMap::prof_harvest()
{
    for (auto& r : prof_pending_) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) { prof_ms_[r.id] += ms; prof_n_[r.id]++; prof_bytes_[r.id] += r.bytes; prof_bytes_run_[r.id] += r.bytes_run; }
        ev_pool_.push_back(r.a); ev_pool_.push_back(r.b);
    }
    prof_pending_.clear();
}

int FusionMap::profile_read(int cap, const char** names, double* ms, long long* launches, double* bytes, double* bytes_run)
{
    std::lock_guard<std::mutex> l(mu_); (void)drain();
    (void)hipSetDevice(device_);
    (void)sync_all();
    prof_harvest();
    int n = 0;
    for (int i = 0; i < K_COUNT && n < cap; i++, n++) {
        names[n] = kernel_name(i); ms[n] = prof_ms_[i]; launches[n] = prof_n_[i]; bytes[n] = prof_bytes_[i];
        if (bytes_run) bytes_run[n] = prof_bytes_run_[i];
    }
    return n;
}

void FusionMap::profile_reset()
{
    std::lock_guard<std::mutex> l(mu_); (void)drain();
    (void)hipSetDevice(device_);
    (void)sync_all();
    prof_harvest();
    for (int i = 0; i < K_COUNT; i++) { prof_ms_[i] = 0; prof_n_[i] = 0; prof_bytes_[i] = 0; prof_bytes_run_[i] = 0; prof_tick_[i] = 0; }
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
    std::lock_guard<std::mutex> l(mu_); (void)drain();
    out[0] = (double)n_with_pixels_; out[1] = px_level0_; out[2] = px_owned_; out[3] = (double)store_.size();
}

void FusionMap::stats(long long* rendered, long long* rejected, long long* dropped, long long* failed)
{
    std::lock_guard<std::mutex> l(mu_); (void)drain();
    if (rendered) *rendered = n_rendered_;
    if (rejected) *rejected = n_rejected_;
    if (failed) *failed = n_failed_;
    std::lock_guard<std::mutex> q(qmu_);
    if (dropped) *dropped = n_dropped_;
}

// ---------------------------------------------------------------- prepare
// the line renderFrame's size / type gate prints (.cpp:319-323)
static void print_frame_mismatch() { std::fprintf(stderr, "MultiBandMap2DCPU::renderFrame: frame.first.cols!=p->_camera.w||frame.first.rows!=p->_camera.h||frame.first.type()!=CV_8UC3\n"); }

// Map2DPrepare::prepare (Map2D.cpp:32-49) + MultiBandMap2DCPUData::prepare
// (.cpp:199-255) + MultiBandMap2DCPU::prepare (.cpp:266-286)
bool FusionMap::prepare(const double plane7[7], const double cam[6], int n, const pf_image* imgs, const double* poses7)
{
    if (!init_ok_) { set_error("prepare: no device"); return false; }
    if (n == 0 || !poses7 || cam[0] <= 0 || cam[1] <= 0 || cam[2] == 0 || cam[3] == 0) {
        std::fprintf(stderr, "Map2D::prepare:Not valid prepare!\n");
        return false;
    }
    Camera c{ cam[0], cam[1], cam[2], cam[3], cam[4], cam[5], 1. / cam[2], 1. / cam[3] };
    const Pose plane = pose_from7(plane7), pinv = inverse(plane);
    double mx[3] = { -1e10, -1e10, -1e10 }, mn[3] = { 1e10, 1e10, 1e10 };
    std::vector<Pose> local(n);
    for (int i = 0; i < n; i++) {
        local[i] = mul(pinv, pose_from7(poses7 + 7 * i));
        for (int k = 0; k < 3; k++) {
            mx[k] = local[i].t[k] > mx[k] ? local[i].t[k] : mx[k];
            mn[k] = local[i].t[k] < mn[k] ? local[i].t[k] : mn[k];
        }
    }
    if (mn[2] * mx[2] <= 0) return false;
    const double maxh = mx[2] > 0 ? mx[2] : -mn[2];
    const double lx = (c.w - c.cx) * c.fxinv - (0 - c.cx) * c.fxinv;
    const double ly = (c.h - c.cy) * c.fyinv - (0 - c.cy) * c.fyinv;
    const double radius = 0.5 * maxh * std::sqrt((lx * lx + ly * ly));
    double length_pixel = opt_.resolution;
    if (!length_pixel) {
        length_pixel = 2 * radius / std::sqrt(c.w * c.w + c.h * c.h);
        length_pixel /= opt_.scale;
    }
    std::printf("Map2D.Resolution=%g\n", length_pixel);
    mn[0] = mn[0] - radius; mn[1] = mn[1] - radius;
    mx[0] = mx[0] + radius; mx[1] = mx[1] + radius;
    double ctr[3];
    for (int k = 0; k < 3; k++) ctr[k] = 0.5 * (mn[k] + mx[k]);
    for (int k = 0; k < 3; k++) { mn[k] = 2 * mn[k] - ctr[k]; mx[k] = 2 * mx[k] - ctr[k]; }
    const double ele_size = kElePixels * length_pixel;
    const int w = (int)std::ceil((mx[0] - mn[0]) / ele_size);
    const int h = (int)std::ceil((mx[1] - mn[1]) / ele_size);
    mx[0] = mn[0] + ele_size * w;
    mx[1] = mn[1] + ele_size * h;

    {
        // drop frames queued against the old preparation (.cpp:362-376 bails on p!=prepared)
        std::unique_lock<std::mutex> q(qmu_);
        for (auto& f : queue_) if (f.slot >= 0) slots_[f.slot].queued = false;
        queue_.clear();
        idle_cv_.wait(q, [this] { return !worker_busy_; });
    }
    std::lock_guard<std::mutex> l(mu_);
    if (!set_device()) return false;
    if (valid_) (void)drain();                 // keyframes fed against the old preparation are rendered into it, as they would have been inside their feed calls
    for (auto& p : pending_) release_slot(p.f);
    pending_.clear();
    HIP_OK(sync_all());
    // the input camera survives prepare(): its table is built for the new output camera first, while a failure can still leave the map as it was
    DevBuf und_table; long long und_uncovered = 0;
    if (und_set_ && !build_undistort_table(und_cam_, c, und_table, &und_uncovered)) return false;
    if (und_set_) { und_table_.release(); und_table_ = und_table; und_uncovered_ = und_uncovered; }
    store_.clear();
    plane_ = plane; plane_inv_ = pinv; cam_ = c;
    length_pixel_ = length_pixel; length_pixel_inv_ = 1. / length_pixel;
    ele_size_ = ele_size; ele_size_inv_ = 1. / ele_size;
    std::memcpy(min_, mn, sizeof(mn)); std::memcpy(max_, mx, sizeof(mx)); std::memcpy(min0_, mn, sizeof(mn));
    w_ = w; h_ = h; off_x_ = off_y_ = 0;
    valid_ = true;
    if (thread_ && imgs) {
        // with a render thread the prepare frames are rendered first (Map2D.cpp:42, .cpp:606-615)
        for (int i = 0; i < n; i++) {
            if (!imgs[i].data) continue;
            // renderFrame's size / type gate (.cpp:319-323), as the threaded feed() applies it: such a frame is never rendered
            if (frame_mismatch(imgs[i].type, imgs[i].cols, imgs[i].rows)) { print_frame_mismatch(); continue; }
            if (und_set_) {
                const int slot = undistort_frame(&imgs[i], false, nullptr);
                if (slot < 0) return false;
                std::lock_guard<std::mutex> q(qmu_);
                slots_[slot].queued = true;
                queue_.push_back({ slot, nullptr, (long)cam_.w * 3, (int)cam_.h, (int)cam_.w, 3, local[i] });
                continue;
            }
            const int cn = imgs[i].type == PF_8UC4 ? 4 : 3;
            const size_t row_bytes = (size_t)imgs[i].cols * cn, step = imgs[i].step ? imgs[i].step : row_bytes;
            if (step < row_bytes || step * (size_t)imgs[i].rows >= (1ull << 31)) { set_error("prepare: bad row step or frame of 2 GiB or more"); return false; }
            const int slot = acquire_slot((size_t)imgs[i].rows * step);
            if (slot < 0 || !upload(&imgs[i], slot)) return false;
            std::lock_guard<std::mutex> q(qmu_);
            slots_[slot].queued = true;
            queue_.push_back({ slot, nullptr, (long)step, imgs[i].rows, imgs[i].cols, cn, local[i] });
        }
        qcv_.notify_all();
    }
    return true;
}

// ------------------------------------------------------------------- feed
int FusionMap::acquire_slot(size_t bytes)
{
    // called with mu_ held.  A slot is reusable once it left the queue and the
    // kernels that read it have completed.
    const size_t limit = (size_t)opt_.max_queue + 4 + (size_t)opt_.lookahead;          // the feed queue, frames in flight, keyframes that wait for their lookahead
    for (int pass = 0; pass < 2; pass++) {
        int oldest_pending = -1;
        for (size_t i = 0; i < slots_.size(); i++) {
            FrameSlot& s = slots_[i];
            { std::lock_guard<std::mutex> q(qmu_); if (s.queued) continue; }
            if (s.pending) {
                if (hipEventQuery(s.consumed) == hipSuccess) s.pending = false;
                else { if (oldest_pending < 0) oldest_pending = (int)i; continue; }
            }
            if (s.cap < bytes) {
                if (s.dev) (void)hipFree(s.dev);
                s.dev = nullptr; s.cap = 0;
                if (hipMalloc((void**)&s.dev, bytes + 64) != hipSuccess) { (void)hipGetLastError(); set_error("frame slot hipMalloc failed"); return -1; }
                s.cap = bytes;
            }
            return (int)i;
        }
        if (slots_.size() < limit) {
            FrameSlot s;
            if (hipMalloc((void**)&s.dev, bytes + 64) != hipSuccess) { (void)hipGetLastError(); set_error("frame slot hipMalloc failed"); return -1; }
            s.cap = bytes;
            if (hipEventCreateWithFlags(&s.consumed, hipEventDisableTiming) != hipSuccess) { set_error("hipEventCreate failed"); return -1; }
            slots_.push_back(s);
            return (int)slots_.size() - 1;
        }
        if (oldest_pending >= 0) { (void)hipEventSynchronize(slots_[oldest_pending].consumed); slots_[oldest_pending].pending = false; }
    }
    set_error("no free frame slot");
    return -1;
}

bool FusionMap::upload(const pf_image* img, int slot)
{
    // One linear, blocking copy of the rows as they lie in the caller's buffer (cv::Mat::step is kept: the kernels
    // take any row step): the caller may release its pixels when feed() returns, and the frame is complete in HBM
    // before the kernel that reads it is enqueued.  The map's streams are non-blocking, so this does not wait for
    // kernels in flight.
    const size_t row = (size_t)img->cols * (img->type == PF_8UC4 ? 4 : 3), step = img->step ? img->step : row;
    const size_t bytes = (size_t)(img->rows - 1) * step + row;          // == frame_bytes(): what the kernels may read
    HIP_OK(hipMemcpy(slots_[slot].dev, img->data, bytes, hipMemcpyHostToDevice));
    last_slot_ = slot; last_bytes_ = bytes;
    return true;
}

// ---- input camera (undistort_plan.hpp, undistort.hip)
// the table of (in, out) as the kernel reads it: rows of undistort_pitch(w) (x, y) pairs.  buf is filled only on success
bool FusionMap::build_undistort_table(const undistort::InCamera& in, const Camera& out, DevBuf& buf, long long* uncovered)
{
    const double out6[6] = { out.w, out.h, out.fx, out.fy, out.cx, out.cy };
    undistort::OutCamera oc;
    if (!undistort::make_out_camera(out6, oc)) { set_error("input camera: the map's camera cannot be an output camera"); return false; }
    const size_t pitch = undistort_pitch(oc.w);
    std::vector<float2> tab;
    try { tab.assign(pitch * (size_t)oc.h, float2{ -1.f, -1.f }); } catch (const std::bad_alloc&) { set_error("input camera: no memory for the remap table"); return false; }
    long long unc = 0;
    for (int y = 0; y < oc.h; y++)
        for (int x = 0; x < oc.w; x++) {
            float2& e = tab[(size_t)y * pitch + x];
            if (!undistort::entry(in, oc, x, y, e.x, e.y)) unc++;
        }
    DevBuf b;
    if (!b.reserve(tab.size() * sizeof(float2))) { (void)hipGetLastError(); set_error("input camera: hipMalloc of the remap table failed"); return false; }
    if (hipMemcpy(b.p, tab.data(), tab.size() * sizeof(float2), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError(); b.release(); set_error("input camera: upload of the remap table failed"); return false;
    }
    buf = b;
    if (uncovered) *uncovered = unc;
    return true;
}

bool FusionMap::set_input_camera(const double* in, int n)
{
    if (!init_ok_) { set_error("set_input_camera: no device"); return false; }
    undistort::InCamera cam;
    if (n != 0 && !undistort::make_camera(in, n, cam)) {
        set_error("set_input_camera: needs 6 (PinHole), 7 (ATAN) or 11 (OpenCV) finite parameters of a valid camera (w, h >= 1, fx, fy != 0)");
        return false;
    }
    std::lock_guard<std::mutex> l(mu_);
    if (!set_device()) return false;
    DevBuf table; long long unc = 0;
    if (n != 0 && valid_ && !build_undistort_table(cam, cam_, table, &unc)) return false;
    // frames that wait (feed queue, lookahead) are undistorted already; the kernels that still read the old table have to finish before it goes
    if (und_table_.p) { HIP_OK(sync_all()); und_table_.release(); }
    und_set_ = n != 0; und_cam_ = cam; und_table_ = table; und_uncovered_ = unc;
    return true;
}

bool FusionMap::input_camera_info(int* rows_in, int* cols_in, long long* uncovered)
{
    std::lock_guard<std::mutex> l(mu_);
    if (!und_set_) return false;
    if (rows_in) *rows_in = und_cam_.h;
    if (cols_in) *cols_in = und_cam_.w;
    if (uncovered) *uncovered = valid_ ? und_uncovered_ : -1;        // -1: no output camera yet
    return true;
}

int FusionMap::undistort_frame(const pf_image* img, bool device_ptr, const FrameProducer* produce)
{
    // called with mu_ held, und_set_ && valid_ (so und_table_ is the table of the two cameras), the frame's size and type checked
    const int cn = img->type == PF_8UC4 ? 4 : 3;
    const size_t row = (size_t)img->cols * cn, step = (img->data && img->step) ? img->step : row;
    if (step < row || step * (size_t)img->rows >= (1ull << 31)) { set_error("feed: row step smaller than a row, or frame of 2 GiB or more"); return -1; }
    const int ow = (int)cam_.w, oh = (int)cam_.h;
    const size_t ostep = (size_t)ow * 3;
    if (frame_bytes(oh, ow, (long)ostep, 3) < 8) { set_error("feed: frame smaller than 8 bytes"); return -1; }       // the warp loads 8 bytes per source row
    if (!und_table_.p) { set_error("feed: the input camera has no table"); return -1; }
    const uint8_t* raw = device_ptr ? (const uint8_t*)img->data : nullptr;
    int scratch = -1;
    // whatever was queued on stream_ for a slot stands between it and its next user
    auto mark = [this](int s) { if (s >= 0) slots_[s].pending = hipEventRecord(slots_[s].consumed, stream_) == hipSuccess; };
    if (!device_ptr) {
        scratch = acquire_slot((size_t)img->rows * step);
        if (scratch < 0) return -1;
        if (img->data) { if (!upload(img, scratch)) return -1; }
        else if (!produce || !(*produce)(slots_[scratch].dev, stream_)) { mark(scratch); return -1; }
        raw = slots_[scratch].dev;
        std::lock_guard<std::mutex> q(qmu_);
        slots_[scratch].queued = true;          // not to be handed out again as the frame's own slot
    }
    const int slot = acquire_slot((size_t)oh * ostep);
    if (scratch >= 0) { std::lock_guard<std::mutex> q(qmu_); slots_[scratch].queued = false; }
    if (slot < 0) { mark(scratch); return -1; }
    launch_undistort(stream_, raw, step, und_cam_.w, und_cam_.h, cn, (const float2*)und_table_.p, slots_[slot].dev, ostep, ow, oh);
    const hipError_t e = hipGetLastError();
    // the scratch slot is free once the kernel has read it; the frame's slot, should the frame be dropped from the feed queue, once it is written
    mark(scratch); mark(slot);
    if (e != hipSuccess) { set_error(std::string("k_undistort: ") + hipGetErrorString(e)); return -1; }
    if (scratch >= 0 && !slots_[scratch].pending) { set_error("feed: hipEventRecord failed"); return -1; }
    return slot;
}

// MultiBandMap2DCPU::feed (.cpp:288-309)
bool FusionMap::feed(const pf_image* img, const double pose7[7], bool device_ptr, const FrameProducer* produce)
{
    if (!init_ok_) { set_error("feed: no device"); return false; }
    Section sec(this, T_FEED);
    QueuedFrame f{};
    { std::lock_guard<std::mutex> q(qmu_); f.seq = feed_seq_++; }
    {
        std::lock_guard<std::mutex> l(mu_);
        if (!valid_) return false;
        if (!set_device()) return false;
        f.pose = mul(plane_inv_, pose_from7(pose7));
        f.slot = -1; f.ext = nullptr;
        if (img) {
            // wrong size/type is reported by renderFrame (.cpp:319-323); keep that order of checks
            f.rows = img->rows; f.cols = img->cols;
            f.cn = img->type == PF_8UC4 ? 4 : 3;     // BGRA frames are accepted as the tracker produces them (row f1)
            if (frame_mismatch(img->type, img->cols, img->rows)) {
                print_frame_mismatch();
                if (!thread_) { n_rejected_++; return false; }
                return true;    // the threaded reference enqueues and fails later on the render thread
            }
            if (und_set_ && (img->data || produce)) {
                // a frame of the input camera: remapped into a slot of its own, and from here on a packed BGR8 host frame of the map's camera
                if (device_ptr && thread_) { set_error("pf_feed_device needs a thread=0 map"); return false; }
                f.slot = undistort_frame(img, device_ptr, produce);
                if (f.slot < 0) return false;
                f.rows = (int)cam_.h; f.cols = (int)cam_.w; f.cn = 3; f.step = (long)cam_.w * 3;
            } else if (img->data) {
                const size_t row_bytes = (size_t)img->cols * f.cn;
                if ((img->step && img->step < row_bytes) || (img->step ? img->step : row_bytes) * (size_t)img->rows >= (1ull << 31)) {
                    set_error("feed: row step smaller than a row, or frame of 2 GiB or more");
                    return false;
                }
                if (frame_bytes(img->rows, img->cols, (long)(img->step ? img->step : row_bytes), f.cn) < 8) {
                    set_error("feed: frame smaller than 8 bytes");      // the warp loads 8 bytes per source row (warp_index.hpp)
                    return false;
                }
                if (device_ptr) {
                    if (thread_) { set_error("pf_feed_device needs a thread=0 map"); return false; }
                    f.ext = (const uint8_t*)img->data; f.step = img->step ? (long)img->step : (long)img->cols * f.cn;
                } else {
                    f.step = img->step ? (long)img->step : (long)img->cols * f.cn;
                    f.slot = acquire_slot((size_t)img->rows * (size_t)f.step);
                    if (f.slot < 0 || !upload(img, f.slot)) return false;
                }
            } else if (produce) {
                f.step = (long)img->cols * f.cn;
                if (frame_bytes(img->rows, img->cols, f.step, f.cn) < 8) { set_error("feed: frame smaller than 8 bytes"); return false; }
                f.slot = acquire_slot((size_t)img->rows * (size_t)f.step);
                if (f.slot < 0 || !(*produce)(slots_[f.slot].dev, stream_)) return false;
                // the producer's work sits on stream_ ahead of the launch that reads the slot; should the frame be dropped from the
                // queue instead, the slot's next user (possibly a blocking upload) has to wait for that work all the same
                HIP_OK(hipEventRecord(slots_[f.slot].consumed, stream_));
                slots_[f.slot].pending = true;
            }
        }
    }
    if (thread_) {
        std::lock_guard<std::mutex> q(qmu_);
        if (f.slot >= 0) slots_[f.slot].queued = true;
        queue_.push_back(f);
        if ((int)queue_.size() > opt_.max_queue) {          // .cpp:302 drop-oldest
            if (queue_.front().slot >= 0) slots_[queue_.front().slot].queued = false;
            queue_.pop_front();
            n_dropped_++;
        }
        qcv_.notify_one();
        return true;
    }
    std::lock_guard<std::mutex> l(mu_);
    return render_frame(f);
}

// ---- frame distribution (pf_dist_feed)
// The ranks that own at least one tile of the canvas this keyframe renders into.  Same geometry as render_frame
// (.cpp:324-394); spreadMap is applied here already -- it is idempotent for the render that follows.
bool FusionMap::frame_needs(const double pose7[7], std::vector<unsigned char>& rank_needs)
{
    std::lock_guard<std::mutex> l(mu_);
    rank_needs.assign((size_t)opt_.shard_count, 0);
    if (!valid_) return false;
    const Pose pose = mul(plane_inv_, pose_from7(pose7));
    double pts[8];
    if (!footprint(cam_, pose, pts)) return true;            // oblique view: nobody renders it (feed will say false)
    Win r;
    if (!canvas_range(pts, r)) return false;
    for (int y = r.y0; y < r.y1; y++)
        for (int x = r.x0; x < r.x1; x++)
            rank_needs[(size_t)tile_owner(opt_.shard_count, opt_.shard_block, x + off_x_, y + off_y_)] = 1;
    return true;
}

// renderFrame's size / type gate (.cpp:319-323) for a frame that arrives through pf_dist_feed: true if the frame was rejected --
// message and counter exactly as feed() has them, and nothing else touched (the reference returns before any geometry)
bool FusionMap::reject_mismatched_frame(const pf_image* desc)
{
    std::lock_guard<std::mutex> l(mu_);
    if (!valid_) return false;
    if (frame_mismatch(desc->type, desc->cols, desc->rows)) {
        print_frame_mismatch();
        n_rejected_++;
        return true;
    }
    return false;
}

int FusionMap::stage_frame(const pf_image* desc, bool upload_host, void** dev, size_t* bytes)
{
    std::lock_guard<std::mutex> l(mu_);
    if (!init_ok_ || !valid_ || !set_device() || thread_) { set_error("stage_frame: needs a prepared thread=0 map"); return -1; }
    const int cn = desc->type == PF_8UC4 ? 4 : 3;
    const size_t row = (size_t)desc->cols * cn, step = desc->step ? desc->step : row;
    if (frame_mismatch(desc->type, desc->cols, desc->rows) || step < row ||
        step * (size_t)desc->rows >= (1ull << 31)) { set_error("stage_frame: frame does not match the camera"); return -1; }
    const int slot = acquire_slot((size_t)desc->rows * step);
    if (slot < 0) return -1;
    if (upload_host) {
        if (!desc->data || !upload(desc, slot)) return -1;
    }
    slots_[slot].queued = true;                                // held until feed_staged
    if (dev) *dev = slots_[slot].dev;
    if (bytes) *bytes = (size_t)(desc->rows - 1) * step + row;
    return slot;
}

bool FusionMap::feed_staged(int slot, const pf_image* desc, const double pose7[7])
{
    if (!init_ok_) return false;
    Section sec(this, T_FEED);
    std::lock_guard<std::mutex> l(mu_);
    if (slot >= 0) { std::lock_guard<std::mutex> q(qmu_); slots_[slot].queued = false; }
    if (!valid_ || !set_device()) return false;
    QueuedFrame f{};
    f.pose = mul(plane_inv_, pose_from7(pose7));
    f.slot = slot; f.ext = nullptr;
    f.rows = desc->rows; f.cols = desc->cols; f.cn = desc->type == PF_8UC4 ? 4 : 3;
    f.step = desc->step ? (long)desc->step : (long)desc->cols * f.cn;
    return render_frame(f);
}

// test hook: the bytes of the most recently uploaded host frame as they lie in HBM
long FusionMap::read_back_last_frame(void* out, size_t cap)
{
    std::lock_guard<std::mutex> l(mu_);
    if (!init_ok_ || last_slot_ < 0 || !set_device()) return -1;
    if (out && cap >= last_bytes_ && hipMemcpy(out, slots_[last_slot_].dev, last_bytes_, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return (long)last_bytes_;
}

unsigned FusionMap::queue_size() { std::lock_guard<std::mutex> q(qmu_); return (unsigned)queue_.size(); }

// MultiBandMap2DCPU::run (.cpp:619-635) without the 10 ms sleep
void FusionMap::worker()
{
    for (;;) {
        QueuedFrame f;
        {
            std::unique_lock<std::mutex> q(qmu_);
            qcv_.wait(q, [this] { return stop_ || !queue_.empty(); });
            if (stop_) return;
            f = queue_.front(); queue_.pop_front();
            worker_busy_ = true;
        }
        {
            std::lock_guard<std::mutex> l(mu_);
            // in; rendered once opt_.lookahead more keyframes are, or ...  (a keyframe lost on the way -- here or in the drain() below -- is
            // counted where it is lost, keyframe_lost(), and the next sync() says so: this thread has nobody to return false to)
            if (valid_ && set_device()) (void)render_frame(f);
            else release_slot(f);
        }
        bool idle;
        { std::lock_guard<std::mutex> q(qmu_); idle = queue_.empty(); }
        if (idle) {                                               // ... now, when nothing else waits in the feed queue: no keyframe is held back for company that may never come
            std::lock_guard<std::mutex> l(mu_);
            (void)drain();
        }
        {
            std::lock_guard<std::mutex> q(qmu_);
            worker_busy_ = false;
        }
        idle_cv_.notify_all();
    }
}

bool FusionMap::sync()
{
    if (!init_ok_) return false;
    if (thread_) {
        std::unique_lock<std::mutex> q(qmu_);
        idle_cv_.wait(q, [this] { return queue_.empty() && !worker_busy_; });
    }
    std::lock_guard<std::mutex> l(mu_);
    if (!set_device()) return false;
    const bool drained = drain();
    // keyframes lost since the last sync() -- in a feed, in a reader's drain, on the render thread or just now: said once, with the message
    // of the newest of them (FusionMap::stats counts them)
    const bool lost = fail_pending_;
    fail_pending_ = false;
    HIP_OK(sync_all());
    prof_harvest();
    if (lost) { set_error(fail_msg_); return false; }
    return drained;
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
        p.lat.map_canvas(w.Minv, w.crows, w.ccols, f.cols, f.rows, single_band_ ? 0 : ((2 << w.L) - 2 + 63) / 64, map_all, cull_margins_);
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
//   new weights   W_i(q) is a convex combination (pyrDown) of level-0 radial weights inside the cell dilated by the pyramid's
//                 support radius 2^(L+1) px, so W_i <= wmax = the largest radial weight the frame can have there;
//   stored ones   every earlier keyframe f whose canvas held the tile left S_i >= W_i^f >= wmin_f (its smallest weight on the same
//                 dilated cell, 0 unless that lies wholly inside f's footprint) -- also when f itself was culled there, for
//                 then S_i > W_i^f.  Tile::wlb[cell] = max over f of wmin_f.
// Bit-exactness is checked, not assumed: every parity test runs with the cull on; PF_CULL=0 turns it off.
// The unit of the cull is a CELL of a tile (64 x 64 pixels, 16 per tile; experiments library, PF_CULL_SUB=2: a quadrant), dilated by the
// pyramid's support radius 2^(L+1) - 2 pixels rounded up to the lattice step (62 -> 64 for five bands, 254 -> 256 for seven).  A tile whose
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
    if (exact_r0 > 0 && prof_on_ && !prof_pending_.empty()) {
        // this launch is bracketed by events: replace the level-0 job's estimated run share in its record by the exact one -- now that
        // the launch is on its way
        const double n0 = owned_tiles * kElePixels * kElePixels, tile_bytes0 = n0 * (4 + E) + (L == 1 ? n0 / 4 * (4 + E) : 0);
        prof_pending_.back().bytes_run += tile_bytes0 * (pl.exact_level0_share(w.owned_all, exact_r0) - run_share[0]);
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
    std::lock_guard<std::mutex> l(mu_); (void)drain();
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

// ------------------------------------------------------------ tile access
bool FusionMap::grid(int dims[4], double geo[6])
{
    std::lock_guard<std::mutex> l(mu_);
    if (!valid_) return false;
    dims[0] = w_; dims[1] = h_; dims[2] = off_x_; dims[3] = off_y_;
    geo[0] = min_[0]; geo[1] = min_[1]; geo[2] = max_[0]; geo[3] = max_[1]; geo[4] = ele_size_; geo[5] = length_pixel_;
    return true;
}

bool FusionMap::map_update_inputs(int ix, int iy, double plane7[7], double mn[2], double* ele, int* x, int* y)
{
    std::lock_guard<std::mutex> l(mu_); (void)drain();
    if (!valid_) return false;
    Tile* t = store_.find(ix, iy);
    if (!t || t->fresh) return false;                            // .cpp:717-718: no pyramid yet
    const int dx = ix - off_x_, dy = iy - off_y_;                // dense index of the draw() loop
    if (dx < 0 || dy < 0 || dx >= w_ || dy >= h_) return false;
    if (opt_.high_quality_show && !single_band_ && (dx == 0 || dy == 0 || dx == w_ - 1 || dy == h_ - 1)) return false;   // inborder
    std::memcpy(plane7, plane_.t, 24); std::memcpy(plane7 + 3, plane_.q, 32);
    mn[0] = min_[0]; mn[1] = min_[1]; *ele = ele_size_; *x = dx; *y = dy;
    return true;
}

int FusionMap::tile_count()
{
    std::lock_guard<std::mutex> l(mu_); (void)drain();
    int n = 0;
    store_.for_each([&](int, int, Tile& t) { if (!t.fresh) n++; });
    return n;
}

int FusionMap::tile_coords(int* xy, int cap)
{
    std::lock_guard<std::mutex> l(mu_); (void)drain();
    std::vector<std::pair<int, int>> v;
    store_.for_each([&](int ix, int iy, Tile& t) { if (!t.fresh) v.push_back({ iy, ix }); });
    std::sort(v.begin(), v.end());
    for (size_t i = 0; i < v.size() && (int)i < cap; i++) { xy[2 * i] = v[i].second; xy[2 * i + 1] = v[i].first; }
    return (int)v.size();
}

bool FusionMap::get_tile_bgra(int ix, int iy, uint8_t* bgra)
{
    std::lock_guard<std::mutex> l(mu_); (void)drain();
    if (!init_ok_ || !single_band_ || !set_device()) return false;
    Tile* t = store_.find(ix, iy);
    if (!t || t->fresh) return false;
    HIP_OK(sync_all());
    HIP_OK(hipMemcpy(bgra, t->base, (size_t)kElePixels * kElePixels * 4, hipMemcpyDeviceToHost));
    return true;
}

bool FusionMap::get_tile_level(int ix, int iy, int level, void* lap, float* w)
{
    std::lock_guard<std::mutex> l(mu_); (void)drain();
    if (!init_ok_ || single_band_ || !set_device()) return false;
    Tile* t = store_.find(ix, iy);
    if (!t || t->fresh || level < 0 || level > band_num_) return false;
    HIP_OK(sync_all());
    const size_t n = (size_t)(kElePixels >> level) * (kElePixels >> level);
    if (lap) HIP_OK(hipMemcpy(lap, t->base + lay_.lap_off[level], n * 3 * (lay_.f32 ? 4 : 2), hipMemcpyDeviceToHost));
    if (w) HIP_OK(hipMemcpy(w, t->base + lay_.w_off[level], n * 4, hipMemcpyDeviceToHost));
    return true;
}

bool FusionMap::halo_pack(int ix, int iy, int dx, int dy, void* dev_out)
{
    std::lock_guard<std::mutex> l(mu_); (void)drain();
    if (!init_ok_ || !set_device()) return false;
    Tile* t = store_.find(ix, iy);
    if (!t || t->fresh) return false;
    launch_halo_pack(stream_, lay_, t->base, dx, dy, dev_out);
    HIP_OK(sync_all());
    return true;
}

bool FusionMap::tile_export(int ix, int iy, void* dev_out)
{
    std::lock_guard<std::mutex> l(mu_); (void)drain();
    if (!init_ok_ || !set_device()) return false;
    Tile* t = store_.find(ix, iy);
    if (!t || t->fresh) return false;
    HIP_OK(hipMemcpyAsync(dev_out, t->base, lay_.slot_bytes, hipMemcpyDeviceToDevice, stream_));
    HIP_OK(sync_all());
    return true;
}

bool FusionMap::tile_import(int ix, int iy, const void* dev_in)
{
    std::lock_guard<std::mutex> l(mu_); (void)drain();
    if (!init_ok_ || !valid_ || !set_device()) return false;
    Tile* t = store_.get_or_create(ix, iy);
    if (!t) return false;
    HIP_OK(hipMemcpyAsync(t->base, dev_in, lay_.slot_bytes, hipMemcpyDeviceToDevice, stream_));
    HIP_OK(sync_all());
    t->fresh = false; t->changed = true;
    for (float& w : t->wlb) w = -1.f;                           // imported pixels: nothing known about their weights
    return true;
}

// ------------------------------------------------------- seam exchange support (dist.cpp)
void FusionMap::list_tiles(std::vector<TileRec>& out)
{
    std::lock_guard<std::mutex> l(mu_); (void)drain();
    out.clear();
    store_.for_each([&](int ix, int iy, Tile& t) { if (!t.fresh) out.push_back({ ix, iy, t.changed ? 1 : 0 }); });
    std::sort(out.begin(), out.end(), [](const TileRec& a, const TileRec& b) { return a.iy != b.iy ? a.iy < b.iy : a.ix < b.ix; });
}

// every strip set of one exchange: one descriptor upload, one launch, no sync (the caller orders its transport after stream_)
bool FusionMap::pack_strips(const std::vector<StripReq>& reqs, void* dev_out)
{
    std::lock_guard<std::mutex> l(mu_); (void)drain();
    if (!init_ok_ || !set_device()) return false;
    if (reqs.empty()) return true;
    if (!settle()) return false;
    std::vector<StripDesc> d(reqs.size());
    for (size_t i = 0; i < reqs.size(); i++) {
        Tile* t = store_.find(reqs[i].ix, reqs[i].iy);
        if (!t || t->fresh) { set_error("pack_strips: tile not held by this rank"); return false; }
        d[i] = { t->base, reqs[i].dx, reqs[i].dy, reqs[i].out_off };
    }
    if (!strip_desc_.reserve(d.size() * sizeof(StripDesc))) return false;
    HIP_OK(hipMemcpyAsync(strip_desc_.p, d.data(), d.size() * sizeof(StripDesc), hipMemcpyHostToDevice, stream_));
    launch_halo_pack_batch(stream_, lay_, (const StripDesc*)strip_desc_.p, (int)d.size(), dev_out);
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(stream_));       // d (pageable) is read by the async copy: one sync per exchange, not per strip
    return true;
}

// whole tiles (pyramids + weights) of this rank, back to back in dev_out, for save()'s gather
bool FusionMap::export_tiles(const std::vector<std::pair<int, int>>& tiles, void* dev_out)
{
    std::lock_guard<std::mutex> l(mu_); (void)drain();
    if (!init_ok_ || !set_device()) return false;
    if (!settle()) return false;
    for (size_t i = 0; i < tiles.size(); i++) {
        Tile* t = store_.find(tiles[i].first, tiles[i].second);
        if (!t || t->fresh) { set_error("export_tiles: tile not held by this rank"); return false; }
        HIP_OK(hipMemcpyAsync((char*)dev_out + i * lay_.slot_bytes, t->base, lay_.slot_bytes, hipMemcpyDeviceToDevice, stream_));
    }
    HIP_OK(hipStreamSynchronize(stream_));
    return true;
}

// the changed tiles among `tiles` blended with remote strips; clears their Ischanged flags (draw(), .cpp:705-742)
bool FusionMap::blend_tiles(const std::vector<std::pair<int, int>>& tiles, const void* const* halo9, uint8_t* bgr)
{
    std::lock_guard<std::mutex> l(mu_); (void)drain();
    if (!init_ok_ || !set_device() || single_band_) return false;
    if (!blend_batch(tiles, halo9, nullptr, bgr)) return false;
    for (auto& t : tiles) { Tile* q = store_.find(t.first, t.second); if (q) q->changed = false; }
    return true;
}

// ------------------------------------------------------------------ output side
// Results leave HBM through a ring of two pinned staging slots: the device-to-host copy of piece k+1 (copy_stream_) runs while
// the host moves piece k from its slot into the caller's (pageable) buffer on a few threads.  A blocking hipMemcpy into
// pageable memory -- what rounds 1-5 did -- moves 12 GB/s on the boxes used; a caller who hands over pinned memory
// (pf_host_alloc) gets the copy straight into it.
static void copy_threads(void* dst, const void* src, size_t bytes, int nthreads)
{
    if (nthreads <= 1 || bytes < ((size_t)4 << 20)) { std::memcpy(dst, src, bytes); return; }
    std::vector<std::thread> th;
    const size_t part = ((bytes / nthreads) + 4095) & ~(size_t)4095;
    for (int i = 1; i < nthreads; i++) {
        const size_t o = part * i;
        if (o >= bytes) break;
        th.emplace_back([=] { std::memcpy((char*)dst + o, (const char*)src + o, std::min(part, bytes - o)); });
    }
    std::memcpy(dst, src, std::min(part, bytes));
    for (auto& t : th) t.join();
}

static bool is_pinned_host(const void* p)
{
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return at.type == hipMemoryTypeHost;
}

bool FusionMap::out_ring_init()
{
    if (out_ring_ok_) return true;
    // (a call that failed half way is finished by the next one: every piece is made once)
    for (int i = 0; i < 2; i++) {
        if (!out_pin_[i]) HIP_OK(hipHostMalloc((void**)&out_pin_[i], kOutSlot, hipHostMallocDefault));
        if (!out_copied_[i]) HIP_OK(hipEventCreateWithFlags(&out_copied_[i], hipEventDisableTiming));
    }
    if (!out_ready_) HIP_OK(hipEventCreateWithFlags(&out_ready_, hipEventDisableTiming));
    if (!copy_stream_) HIP_OK(hipStreamCreateWithFlags(&copy_stream_, hipStreamNonBlocking));
    out_ring_ok_ = true;
    const unsigned hc = std::thread::hardware_concurrency();
    out_threads_ = std::getenv("PF_COPY_THREADS") ? std::atoi(std::getenv("PF_COPY_THREADS")) : (int)std::min(8u, std::max(1u, hc / 2));
    return true;
}

// `pieces` = (host destination, device source, bytes) in the order they become ready; everything they read has been queued on
// stream_ before the call.  Pieces are cut to the slot size.
bool FusionMap::download(const std::vector<OutPiece>& pieces)
{
    if (pieces.empty()) return true;
    if (!out_ring_init()) return false;
    HIP_OK(hipEventRecord(out_ready_, stream_));
    HIP_OK(hipStreamWaitEvent(copy_stream_, out_ready_, 0));
    struct Part { char* dst; const char* src; size_t n; bool direct; };
    std::vector<Part> parts;
    for (auto& pc : pieces) {
        const bool direct = is_pinned_host(pc.dst);
        for (size_t o = 0; o < pc.bytes; o += kOutSlot) parts.push_back({ (char*)pc.dst + o, (const char*)pc.src + o, std::min(kOutSlot, pc.bytes - o), direct });
    }
    int k = 0;                                  // staged parts issued so far
    long prev = -1; int prev_slot = 0;          // staged part whose bytes still sit in its slot
    auto drain = [&]() -> bool {
        if (prev < 0) return true;
        HIP_OK(hipEventSynchronize(out_copied_[prev_slot]));
        copy_threads(parts[prev].dst, out_pin_[prev_slot], parts[prev].n, out_threads_);
        prev = -1;
        return true;
    };
    for (size_t i = 0; i < parts.size(); i++) {
        const Part& pt = parts[i];
        if (pt.direct) { HIP_OK(hipMemcpyAsync(pt.dst, pt.src, pt.n, hipMemcpyDeviceToHost, copy_stream_)); continue; }
        const int slot = k++ & 1;               // its previous tenant (two staged parts ago) has been drained: drain() runs once per staged part
        HIP_OK(hipMemcpyAsync(out_pin_[slot], pt.src, pt.n, hipMemcpyDeviceToHost, copy_stream_));
        HIP_OK(hipEventRecord(out_copied_[slot], copy_stream_));
        if (!drain()) return false;             // the part before this one, while this one is on the wire
        prev = (long)i; prev_slot = slot;
    }
    if (!drain()) return false;
    HIP_OK(hipStreamSynchronize(copy_stream_));
    return true;
}

// ------------------------------------------------------------------ blend
// Ele::blend (.cpp:77-146) for a list of tiles.  halo9 (nullptr, or 9 device pointers per tile) substitutes packed strip
// sets for neighbours held by other shards.  Results land in tile order (a tile that does not exist leaves the caller's
// bytes alone).  One launch of the fused collapse kernel per kBlendLaunch tiles, "blend with neighbours" and "blend by self"
// tiles side by side in it; the pixels come back through download().  level > 0: the view of that pyramid level (collapse_level.hip),
// E x E pixels a tile with E = 256 >> level; no halo strips and no JPEG streams there.
// The nine sources of Ele::blend's 3 x 3 assembly for tile (ix, iy) (.cpp:93-117; row-major, [4] = the tile itself): a neighbour comes
// from the store, otherwise from its packed halo strip set (halo: nullptr or the tile's 9 device pointers; bit j of strips), otherwise
// there are "no neighbours": false, and the tile is blended by itself (.cpp:131-145).  hq: HighQualityShow
static bool blend_sources(TileStore& store, bool hq, int ix, int iy, const void* const* halo, const void* src[9], unsigned& strips)
{
    strips = 0;
    if (!hq) return false;
    for (int dy = -1; dy <= 1; dy++)
        for (int dx = -1; dx <= 1; dx++) {
            const int j = 3 * (dy + 1) + dx + 1;
            Tile* n = store.find(ix + dx, iy + dy);
            if (n && !n->fresh) src[j] = n->base;
            else if (halo && halo[j]) { src[j] = halo[j]; strips |= 1u << j; }
            else return false;
        }
    return true;
}

bool FusionMap::blend_batch(const std::vector<std::pair<int, int>>& tiles, const void* const* halo9, void* raw_host, uint8_t* bgr_host, TileJpeg* jpeg, int level)
{
    Section sec(this, T_UPDATE_TEXTURE);
    if (level > 0 && (halo9 || jpeg)) { set_error("blend: halo strips and JPEG streams exist at level 0 only"); return false; }
#if PF_EXPERIMENTS
    static const bool per_level = exp_env("PF_BLEND_PER_LEVEL") != nullptr;
    if (per_level && !jpeg && level == 0) return blend_batch_per_level(tiles, halo9, raw_host, bgr_host);
#endif
    const bool want_bgr = bgr_host || jpeg;
    if (jpeg) { jpeg->used = 0; jpeg->offsets[0] = 0; }
    const int nl = band_num_ + 1;
    const size_t es = lay_.f32 ? 4 : 2, px = 3 * es;
    const size_t tile_px = (size_t)(kElePixels >> level) * (kElePixels >> level);
    if (!settle()) return false;                  // the upper levels of the last frames are still pending: run them first (stream order)
    // algorithmic bytes of one blended tile: its own Laplacians and the weights of the result's level read, the result written, plus
    // the ring of neighbour pixels the crop depends on at the levels above (pyrUp reaches one pixel per level: collapse_fused.hip)
    double tile_bytes[2] = { 0, 0 };
    for (int nb = 0; nb < 2; nb++) {
        double b = (double)tile_px * 4 + (raw_host ? (double)tile_px * px : 0) + (want_bgr ? (double)tile_px * 3 : 0);
        int lo = 0, hi = (kElePixels >> level) - 1;
        for (int i = level; i < nl; i++) {
            const int ts = kElePixels >> i;
            if (i > level) { lo = (lo - 1) >> 1; hi = (hi >> 1) + 1; }        // relative to the tile's own square
            const int bd = nb ? 1 << (nl - 1 - i) : 0, l = std::max(lo, -bd), h = std::min(hi, ts - 1 + bd);
            b += (double)(h - l + 1) * (h - l + 1) * px;
            (void)ts;
        }
        tile_bytes[nb] = b;
    }
    constexpr size_t kBlendLaunch = 4096;         // tiles per launch: bounds the result buffers in HBM (BGR8: 805 MB; fp32 raw: 3.2 GB)
    for (size_t c0 = 0; c0 < tiles.size(); c0 += kBlendLaunch) {
        const size_t cn = std::min(kBlendLaunch, tiles.size() - c0);
        std::vector<BlendJob> jobs; jobs.reserve(cn);
        double bytes = 0;
        for (size_t t = c0; t < c0 + cn; t++) {
            Tile* self = store_.find(tiles[t].first, tiles[t].second);
            if (!self || self->fresh) continue;
            BlendJob jb{}; const void* src[9]; unsigned strips;
            const bool all = blend_sources(store_, opt_.high_quality_show != 0, tiles[t].first, tiles[t].second, halo9 ? halo9 + 9 * t : nullptr, src, strips);
            if (all) { for (int j = 0; j < 9; j++) jb.src[j] = (uint64_t)(uintptr_t)src[j]; jb.strip_mask = strips; }
            jb.src[4] = (uint64_t)(uintptr_t)self->base;
            jb.border = all ? 1 : 0; jb.out = (int)(t - c0);
            jobs.push_back(jb);
            bytes += tile_bytes[jb.border];
        }
        if (jobs.empty()) { if (jpeg) for (size_t t = c0; t < c0 + cn; t++) jpeg->offsets[t + 1] = jpeg->used; continue; }
        if (raw_host && !blend_out_raw_.reserve(tile_px * px * cn)) return false;
        if (want_bgr && !blend_out_bgr_.reserve(tile_px * 3 * cn)) return false;
        if (!blend_src_.reserve(jobs.size() * sizeof(BlendJob))) return false;
        HIP_OK(hipMemcpyAsync(blend_src_.p, jobs.data(), jobs.size() * sizeof(BlendJob), hipMemcpyHostToDevice, stream_));
        prof_begin(level ? K_BLEND_LEVEL : K_BLEND_FUSED, bytes);
        if (level) launch_blend_level(stream_, lay_, level, (const BlendJob*)blend_src_.p, (int)jobs.size(), raw_host ? blend_out_raw_.p : nullptr,
                                      want_bgr ? (uint8_t*)blend_out_bgr_.p : nullptr);
        else launch_blend_fused(stream_, lay_, (const BlendJob*)blend_src_.p, (int)jobs.size(), raw_host ? blend_out_raw_.p : nullptr,
                                want_bgr ? (uint8_t*)blend_out_bgr_.p : nullptr);
        prof_end();
        HIP_OK(hipGetLastError());
        if (jpeg) {
            // one encode pass over the launch's tiles where they lie in HBM; only the streams come back.  A tile without
            // pyramid has no job: its range is empty
            std::vector<int> slots(jobs.size());
            for (size_t a = 0; a < jobs.size(); a++) slots[a] = jobs[a].out;
            std::vector<size_t> off(jobs.size() + 1);
            if (!jpeg_enc_.encode(blend_out_bgr_.p, (int)jobs.size(), slots.data(), tile_px * 3, kElePixels, kElePixels, (size_t)kElePixels * 3, jpeg->quality, off.data(), stream_)) return false;
            if (jpeg->used + off.back() > jpeg->cap) {
                set_error("pf_blend_tiles_jpeg: the streams need more than the " + std::to_string(jpeg->cap) + " bytes of the buffer");
                HIP_OK(hipStreamSynchronize(stream_));
                return false;
            }
            if (!jpeg_enc_.fetch(jpeg->out + jpeg->used, stream_)) return false;          // returns with the stream drained: jobs (pageable) have been read
            size_t a = 0;
            for (size_t t = c0; t < c0 + cn; t++) {
                if (a < jobs.size() && (size_t)jobs[a].out == t - c0) a++;
                jpeg->offsets[t + 1] = jpeg->used + off[a];
            }
            jpeg->used += off.back();
            continue;
        }
        // runs of tiles that exist, each one piece per output
        std::vector<OutPiece> pieces;
        for (size_t a = 0; a < jobs.size();) {
            size_t b = a + 1;
            while (b < jobs.size() && jobs[b].out == jobs[b - 1].out + 1) b++;
            const size_t r0 = (size_t)jobs[a].out, n = b - a;
            if (bgr_host) pieces.push_back({ bgr_host + (c0 + r0) * tile_px * 3, (char*)blend_out_bgr_.p + r0 * tile_px * 3, n * tile_px * 3 });
            if (raw_host) pieces.push_back({ (char*)raw_host + (c0 + r0) * tile_px * px, (char*)blend_out_raw_.p + r0 * tile_px * px, n * tile_px * px });
            a = b;
        }
        if (!download(pieces)) return false;      // also orders the next launch's job upload and result buffers after this one's readers
        HIP_OK(hipStreamSynchronize(stream_));    // jobs (pageable) were read by an async copy
    }
    return true;
}

#if PF_EXPERIMENTS
// The per-level form of rounds 1-5 (A/B partner and second opinion of the fused kernel): padded squares per level in HBM,
// one launch per reference op, one blocking device-to-host copy per 128-tile chunk.
bool FusionMap::blend_batch_per_level(const std::vector<std::pair<int, int>>& tiles, const void* const* halo9, void* raw_host, uint8_t* bgr_host)
{
    const int nl = band_num_ + 1, L = band_num_;
    const size_t es = lay_.f32 ? 4 : 2, px = 3 * es;
    const size_t tile_px = (size_t)kElePixels * kElePixels;
    constexpr size_t kChunk = 128;
    if (!settle()) return false;                  // the upper levels of the last frames are still pending: run them first (stream order)
    for (size_t c0 = 0; c0 < tiles.size(); c0 += kChunk) {
        const size_t cn = std::min(kChunk, tiles.size() - c0);
        if (raw_host && !blend_out_raw_.reserve(tile_px * px * cn)) return false;
        if (bgr_host && !blend_out_bgr_.reserve(tile_px * 3 * cn)) return false;
        std::vector<char> present(cn, 0);
        // group the chunk's tiles by mode: full 3x3 available (border = 1<<(nl-1-i)) or self (border 0)
        for (int mode = 0; mode < 2; mode++) {
            std::vector<BlendSrc> srcs;
            std::vector<int> idx;
            for (size_t t = c0; t < c0 + cn; t++) {
                Tile* self = store_.find(tiles[t].first, tiles[t].second);
                if (!self || self->fresh) continue;
                BlendSrc nb[9] = {}; const void* src[9]; unsigned strips;
                const bool all = blend_sources(store_, opt_.high_quality_show != 0, tiles[t].first, tiles[t].second, halo9 ? halo9 + 9 * t : nullptr, src, strips);
                if ((all ? 0 : 1) != mode) continue;
                if (all) for (int j = 0; j < 9; j++) nb[j] = { src[j], (int)((strips >> j) & 1u) };
                else nb[4] = { self->base, 0 };
                srcs.insert(srcs.end(), nb, nb + 9);
                idx.push_back((int)(t - c0));
                present[t - c0] = 1;
            }
            const int batch = (int)idx.size();
            if (!batch) continue;
            const int b0 = mode == 0 ? (1 << (nl - 1)) : 0;
            const size_t src_bytes = srcs.size() * sizeof(BlendSrc), idx_off = (src_bytes + 255) / 256 * 256;
            if (!blend_src_.reserve(idx_off + idx.size() * sizeof(int))) return false;
            HIP_OK(hipMemcpyAsync(blend_src_.p, srcs.data(), src_bytes, hipMemcpyHostToDevice, stream_));
            HIP_OK(hipMemcpyAsync((char*)blend_src_.p + idx_off, idx.data(), idx.size() * sizeof(int), hipMemcpyHostToDevice, stream_));
            size_t stride[kMaxLevels];
            for (int i = 0; i < nl; i++) {
                const int b = mode == 0 ? (1 << (nl - 1 - i)) : 0, side = (kElePixels >> i) + 2 * b;
                stride[i] = (((size_t)side * side * px + 255) / 256) * 256;
                if (!blend_lv_[i].reserve(stride[i] * batch)) return false;
            }
            const BlendSrc* dsrc = (const BlendSrc*)blend_src_.p;
            for (int i = 0; i < nl; i++) {
                const int b = mode == 0 ? (1 << (nl - 1 - i)) : 0, side = (kElePixels >> i) + 2 * b;
                prof_begin(K_BLEND_GATHER, (double)side * side * px * 2 * batch);
                launch_blend_gather(stream_, lay_, i, b, dsrc, blend_lv_[i].p, stride[i], batch);
                prof_end();
            }
            for (int i = L; i > 0; i--) {
                const int b = mode == 0 ? (1 << (nl - i)) : 0, side = (kElePixels >> (i - 1)) + 2 * b;
                prof_begin(K_COLLAPSE, (double)side * side * px * 2.25 * batch);
                launch_collapse(stream_, lay_.f32, blend_lv_[i - 1].p, stride[i - 1], blend_lv_[i].p, stride[i], side, side, batch);
                prof_end();
            }
            prof_begin(K_BLEND_FINISH, (double)tile_px * (px + 4 + 3) * batch);
            launch_blend_finish(stream_, lay_, blend_lv_[0].p, stride[0], b0, dsrc, raw_host ? blend_out_raw_.p : nullptr,
                                bgr_host ? (uint8_t*)blend_out_bgr_.p : nullptr, batch, (const int*)((char*)blend_src_.p + idx_off));
            prof_end();
            HIP_OK(hipStreamSynchronize(stream_));              // srcs / idx are reused by the other mode
        }
        // one copy per chunk (tiles that do not exist keep the caller's bytes: copy the runs that do)
        size_t r0 = 0;
        while (r0 < cn) {
            while (r0 < cn && !present[r0]) r0++;
            size_t r1 = r0;
            while (r1 < cn && present[r1]) r1++;
            if (r1 > r0) {
                if (raw_host) HIP_OK(hipMemcpy((char*)raw_host + (c0 + r0) * tile_px * px, (char*)blend_out_raw_.p + r0 * tile_px * px, (r1 - r0) * tile_px * px, hipMemcpyDeviceToHost));
                if (bgr_host) HIP_OK(hipMemcpy(bgr_host + (c0 + r0) * tile_px * 3, (char*)blend_out_bgr_.p + r0 * tile_px * 3, (r1 - r0) * tile_px * 3, hipMemcpyDeviceToHost));
            }
            r0 = r1;
        }
    }
    return true;
}

#endif

// a single-band tile's pixels (BGRA, Map2DCPU) as the three bytes the outputs carry
static void bgra_to_bgr(const uint8_t* bgra, uint8_t* bgr, size_t n)
{
    for (size_t i = 0; i < n; i++) { bgr[3 * i] = bgra[4 * i]; bgr[3 * i + 1] = bgra[4 * i + 1]; bgr[3 * i + 2] = bgra[4 * i + 2]; }
}

bool FusionMap::blend_tile(int ix, int iy, void* raw, uint8_t* bgr, const void* const* halo)
{
    if (single_band_) {          // the Map2DCPU tile is displayable as is (glTexImage2D GL_BGRA, Map2DCPU.cpp:497-503)
        std::vector<uint8_t> px((size_t)kElePixels * kElePixels * 4);
        if (!get_tile_bgra(ix, iy, px.data())) return false;
        if (raw) std::memcpy(raw, px.data(), px.size());
        if (bgr) bgra_to_bgr(px.data(), bgr, (size_t)kElePixels * kElePixels);
        return true;
    }
    std::lock_guard<std::mutex> l(mu_); (void)drain();
    if (!init_ok_ || !set_device()) return false;
    Tile* t = store_.find(ix, iy);
    if (!t || t->fresh) return false;
    std::vector<std::pair<int, int>> one{ { ix, iy } };
    return blend_batch(one, halo, raw, bgr);
}

bool FusionMap::blend_list(const std::vector<std::pair<int, int>>& tiles, uint8_t* bgr) { return blend_list_level(tiles, 0, bgr, nullptr); }

// The views of pyramid level `level` (pf_blend_tiles_level, pf_blend_changed_level, pf_save_to_memory_level): which levels a map has
bool FusionMap::level_ok(const char* who, int level)
{
    const int top = single_band_ ? 0 : band_num_;
    if (level < 0 || level > top) {
        set_error(std::string(who) + ": level " + std::to_string(level) + " is outside 0 .. " + std::to_string(top) +
                  (single_band_ ? " (a single-band map holds no pyramid)" : ""));
        return false;
    }
    if (level > 0 && opt_.shard_count > 1) { set_error(std::string(who) + ": a sharded map (shard_count > 1) has views of level 0 only"); return false; }
    return true;
}

// pf_blend_tiles_level: the 8U and / or the raw view of the tiles, at any level.  blend_list (pf_blend_tiles) is its level 0, 8U only
bool FusionMap::blend_list_level(const std::vector<std::pair<int, int>>& tiles, int level, uint8_t* bgr, void* raw)
{
    if (!level_ok("pf_blend_tiles_level", level)) return false;
    if (single_band_) {          // level 0: the Map2DCPU tile is displayable as is (see blend_tile), raw is its four bytes a pixel; a tile that does not exist keeps the buffer's bytes
        const size_t n = (size_t)kElePixels * kElePixels;
        for (size_t i = 0; i < tiles.size(); i++)
            (void)blend_tile(tiles[i].first, tiles[i].second, raw ? (char*)raw + i * n * 4 : nullptr, bgr ? bgr + i * n * 3 : nullptr, nullptr);
        return init_ok_;
    }
    std::lock_guard<std::mutex> l(mu_); (void)drain();
    if (!init_ok_ || !set_device()) return false;
    return blend_batch(tiles, nullptr, raw, bgr, nullptr, level);
}

bool FusionMap::blend_list_jpeg(const std::vector<std::pair<int, int>>& tiles, int quality, uint8_t* out, size_t cap, size_t* offsets)
{
    if (single_band_) {          // the Map2DCPU tile is displayable as is (see blend_tile): assembled on the host, the host encoder
        std::vector<uint8_t> px((size_t)kElePixels * kElePixels * 3), stream;
        offsets[0] = 0;
        for (size_t i = 0; i < tiles.size(); i++) {
            stream.clear();
            if (blend_tile(tiles[i].first, tiles[i].second, nullptr, px.data(), nullptr)) jenc::encode_bgr(px.data(), kElePixels, kElePixels, (size_t)kElePixels * 3, quality, stream);
            if (offsets[i] + stream.size() > cap) { set_error("pf_blend_tiles_jpeg: the streams need more than the " + std::to_string(cap) + " bytes of the buffer"); return false; }
            std::memcpy(out + offsets[i], stream.data(), stream.size());
            offsets[i + 1] = offsets[i] + stream.size();
        }
        return init_ok_;
    }
    std::lock_guard<std::mutex> l(mu_); (void)drain();
    if (!init_ok_ || !set_device()) return false;
    TileJpeg tj{ quality, out, cap, offsets };
    return blend_batch(tiles, nullptr, nullptr, nullptr, &tj);
}

// the draw() loop's texture refresh (.cpp:705-742) without GL; level > 0: the same tiles as views of that level, (256 >> level)^2 x 3 bytes each
int FusionMap::blend_changed(int* xy, uint8_t* bgr, int cap, int level)
{
    if (!level_ok("pf_blend_changed_level", level)) return 0;
    std::lock_guard<std::mutex> l(mu_); (void)drain();
    if (!init_ok_ || !set_device()) return 0;
    std::vector<std::pair<int, int>> v;
    store_.for_each([&](int ix, int iy, Tile& t) { if (!t.fresh && t.changed) v.push_back({ iy, ix }); });
    std::sort(v.begin(), v.end());
    if ((int)v.size() > cap) v.resize(cap);
    std::vector<std::pair<int, int>> tiles;
    for (auto& p : v) tiles.push_back({ p.second, p.first });
    if (tiles.empty()) return 0;
    // bound the scratch: 64 tiles per batch
    const size_t tile_px = (size_t)kElePixels * kElePixels * 3;
    if (single_band_) {
        if (sync_all() != hipSuccess) return 0;
        std::vector<uint8_t> px((size_t)kElePixels * kElePixels * 4);
        for (size_t i = 0; i < tiles.size(); i++) {
            Tile* t = store_.find(tiles[i].first, tiles[i].second);
            if (hipMemcpy(px.data(), t->base, px.size(), hipMemcpyDeviceToHost) != hipSuccess) return 0;
            bgra_to_bgr(px.data(), bgr + i * tile_px, (size_t)kElePixels * kElePixels);
            xy[2 * i] = tiles[i].first; xy[2 * i + 1] = tiles[i].second;
            t->changed = false;
        }
        return (int)tiles.size();
    }
    if (sync_all() != hipSuccess || !blend_batch(tiles, nullptr, nullptr, bgr, nullptr, level)) return 0;
    for (size_t i = 0; i < tiles.size(); i++) {
        xy[2 * i] = tiles[i].first; xy[2 * i + 1] = tiles[i].second;
        store_.find(tiles[i].first, tiles[i].second)->changed = false;
    }
    return (int)tiles.size();
}

// ------------------------------------------------------------------- save
// MultiBandMap2DCPU::save (.cpp:779-847): paste all tiles per level, collapse
// the whole mosaic once, 8U, background where level-0 weight is 0.  Everything between the extent and the hand-over of the
// pixels happens under one hold of mu_: the buffer a target is given and the mosaic written into it have the same extent.
bool FusionMap::save_mosaic(SaveTarget& t, const std::vector<ForeignTile>* foreign)
{
    std::lock_guard<std::mutex> l(mu_); (void)drain();
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
        return download(pieces);
    }
    // the mosaic stays where the collapse left it
    if (t.route == SaveRoute::DeviceTiff) {        // overviews, empty test and tile streams are made from it there; the masks from the table
        TiffDevice::Mask mk;
        mk.dev_table = (const uint64_t*)mosaic_table_.p; mk.wx = wx; mk.wy = wy; mk.w_off = lay_.w_off[0];
        return tiff_dev_.write(t.name, blend_out_bgr_.p, t.rows, t.cols, (size_t)t.cols * 3, t.quality, opt_.bg_color, t.transform, t.force_bigtiff, jpeg_enc_, stream_,
                               t.masked ? &mk : nullptr);
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
    if (route == SaveRoute::HostImage && !write_image_file(filename, img.data(), t.rows, t.cols)) return false;
    std::printf("Resolution:[%d %d]\n", t.cols, t.rows);
    return true;
}

// ------------------------------------------------------------------ map merge
// DESIGN.md section 4, "Merging maps".  Canvases are tile aligned: a keyframe that touches a tile covers all of it at every level, so the
// map fed dst's keyframes and then src's is, tile by tile (stable coordinates), the render's select of src's tile into dst's -- src in
// the place of the newer keyframe: `>=` for the pyramids, `<` on alpha for the single band, a copy where dst has no pyramid yet.
void FusionMap::wait_worker_idle()
{
    if (!thread_) return;
    std::unique_lock<std::mutex> q(qmu_);
    idle_cv_.wait(q, [this] { return queue_.empty() && !worker_busy_; });
}

// Stable tile coordinates are one frame in two maps exactly when min0_ and ele_size_ are the same bits; the rest is what makes the tiles'
// content comparable.  who: the caller, for the message
bool FusionMap::merge_compatible(const char* who, bool single, int pyr, int bands, int weight_type, const double plane7[7], const double cam6[6],
                                 const double min0[3], double ele_size, double length_pixel)
{
    const char* why = nullptr;
    double mine7[7]; std::memcpy(mine7, plane_.t, 24); std::memcpy(mine7 + 3, plane_.q, 32);
    if (single != single_band_) why = "map types differ";
    else if (pyr != pyramid_type()) why = "pyramid types differ";
    else if (bands != band_num_) why = "band numbers differ";
    else if (weight_type != opt_.weight_type) why = "weight types differ";
    else if (std::memcmp(plane7, mine7, sizeof(mine7)) != 0) why = "planes differ";
    else if (std::memcmp(cam6, &cam_, 6 * sizeof(double)) != 0) why = "cameras differ";
    else if (std::memcmp(min0, min0_, sizeof(min0_)) != 0 || std::memcmp(&ele_size, &ele_size_, 8) != 0 || std::memcmp(&length_pixel, &length_pixel_, 8) != 0)
        why = "the maps were prepared differently (tile coordinates are not one frame)";
    if (why) { set_error(std::string(who) + ": " + why); return false; }
    return true;
}

// spreadMap towards another map's grid, in whole tiles of the common frame (not through plane coordinates: the two min_ were reached by
// different chains of min + ele_size * k and may differ in the last bit, which tile_range's floor would turn into a tile)
void FusionMap::grow_to(int sx0, int sy0, int sx1, int sy1)
{
    const Win r{ sx0 - off_x_, sx1 - off_x_, sy0 - off_y_, sy1 - off_y_ };
    if (r.x0 < 0 || r.y0 < 0 || r.x1 > w_ || r.y1 > h_) { Section sec(this, T_SPREAD); spread_tiles(r); }
}

bool FusionMap::merge_items(const std::vector<MergeItem>& items)
{
    last_merge_[0] = (double)items.size(); last_merge_[1] = last_merge_[2] = 0; last_merge_[3] = -1; last_merge_[4] = (double)lay_.slot_bytes;
    if (items.empty()) return true;
    // the missing tiles first: when the store cannot grow nothing has been merged
    size_t missing = 0;
    for (auto& it : items) missing += store_.find(it.ix, it.iy) == nullptr;
    if (missing && !store_.reserve(missing)) return false;
    std::vector<Tile*> tiles(items.size());
    for (size_t i = 0; i < items.size(); i++)
        if (!(tiles[i] = store_.get_or_create(items[i].ix, items[i].iy))) return false;
    if (!settle()) return false;                 // what was rendered into the slots comes first on stream_
    std::vector<MergePair> pairs(items.size());
    size_t n_fresh = 0;
    for (size_t i = 0; i < items.size(); i++) {
        pairs[i] = MergePair{ (uint64_t)(uintptr_t)tiles[i]->base, (uint64_t)(uintptr_t)items[i].src, tiles[i]->fresh ? 1u : 0u, 0u };
        n_fresh += tiles[i]->fresh;
    }
    if (!merge_table_.reserve(pairs.size() * sizeof(MergePair))) return false;
    unsigned long long* won = nullptr;
    if (merge_count_) {
        if (!merge_won_.reserve(sizeof(unsigned long long))) return false;
        won = (unsigned long long*)merge_won_.p;
        HIP_OK(hipMemsetAsync(won, 0, sizeof(unsigned long long), stream_));
    }
    for (auto& e : merge_ev_) if (!e) HIP_OK(hipEventCreate(&e));
    HIP_OK(hipMemcpyAsync(merge_table_.p, pairs.data(), pairs.size() * sizeof(MergePair), hipMemcpyHostToDevice, stream_));
    HIP_OK(hipEventRecord(merge_ev_[0], stream_));
    for (size_t o = 0; o < pairs.size(); o += kMergeBatch) {
        launch_merge(stream_, lay_, single_band_, (const MergePair*)merge_table_.p + o, (int)std::min<size_t>(kMergeBatch, pairs.size() - o), won);
        HIP_OK(hipGetLastError());
    }
    HIP_OK(hipEventRecord(merge_ev_[1], stream_));
    HIP_OK(sync_all());                          // the table (pageable) and the caller's slots are free again when this returns
    float ms = 0;
    HIP_OK(hipEventElapsedTime(&ms, merge_ev_[0], merge_ev_[1]));
    last_merge_[1] = (double)n_fresh; last_merge_[2] = ms;
    if (won) { unsigned long long v = 0; HIP_OK(hipMemcpy(&v, won, sizeof(v), hipMemcpyDeviceToHost)); last_merge_[3] = (double)v; }
    // The select only raises weights: both maps' lower bounds stay valid for the merged tile and the larger one holds.  A tile that had no
    // pyramid takes src's bounds; bounds nobody vouches for leave an existing tile's alone and a new tile without any
    for (size_t i = 0; i < items.size(); i++) {
        Tile* t = tiles[i];
        for (int c = 0; c < 16; c++) {
            float b = items[i].wlb ? items[i].wlb[c] : -1.f;
            if (!std::isfinite(b)) b = -1.f;
            t->wlb[c] = t->fresh ? b : std::max(t->wlb[c], b);
        }
        t->fresh = false; t->changed = true;
    }
    return true;
}

void FusionMap::merge_stats(int count_stores, double out[6])
{
    std::lock_guard<std::mutex> l(mu_);
    if (count_stores >= 0) merge_count_ = count_stores != 0;
    if (out) std::memcpy(out, last_merge_, sizeof(last_merge_));
}

bool FusionMap::merge_from(FusionMap& src)
{
    if (&src == this) { set_error("merge: a map cannot be merged into itself"); return false; }
    if (!init_ok_ || !src.init_ok_) { set_error("merge: no device"); return false; }
    wait_worker_idle(); src.wait_worker_idle();      // thread = 1: what sits in the feed queues is rendered first
    std::mutex& m1 = this < &src ? mu_ : src.mu_;
    std::mutex& m2 = this < &src ? src.mu_ : mu_;
    std::lock_guard<std::mutex> l1(m1), l2(m2);
    if (!valid_ || !src.valid_) { set_error("merge: both maps must be prepared"); return false; }
    if (opt_.shard_count > 1 || src.opt_.shard_count > 1) { set_error("merge: sharded maps are not merged"); return false; }
    if (device_ != src.device_) { set_error("merge: the maps live on different devices (move the slots and use pf_merge_tiles)"); return false; }
    double plane7[7]; std::memcpy(plane7, src.plane_.t, 24); std::memcpy(plane7 + 3, src.plane_.q, 32);
    if (!merge_compatible("merge", src.single_band_, src.pyramid_type(), src.band_num_, src.opt_.weight_type, plane7, &src.cam_.w, src.min0_, src.ele_size_, src.length_pixel_)) return false;
    if (!set_device()) return false;
    const bool d1 = drain(), d2 = src.drain();       // the lookahead windows of both
    if (!d1 || !d2) return false;
    if (!src.settle()) return false;
    HIP_OK(src.sync_all());                          // src's streams are done before this map's stream reads src's slots
    std::vector<std::pair<std::pair<int, int>, Tile*>> held;
    src.store_.for_each([&](int ix, int iy, Tile& t) { if (!t.fresh) held.push_back({ { iy, ix }, &t }); });
    std::sort(held.begin(), held.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
    grow_to(src.off_x_, src.off_y_, src.off_x_ + src.w_, src.off_y_ + src.h_);
    std::vector<MergeItem> items;
    items.reserve(held.size());
    for (auto& h : held) items.push_back(MergeItem{ h.first.second, h.first.first, h.second->base, h.second->wlb });
    return merge_items(items);
}

bool FusionMap::merge_tiles(int n, const int* xy, const void* const* dev_slots, const float* wlb16)
{
    if (!init_ok_) { set_error("merge_tiles: no device"); return false; }
    if (n < 0 || (n > 0 && (!xy || !dev_slots))) { set_error("merge_tiles: bad arguments"); return false; }
    wait_worker_idle();
    std::lock_guard<std::mutex> l(mu_);
    if (!valid_) { set_error("merge_tiles: the map is not prepared"); return false; }
    if (opt_.shard_count > 1) { set_error("merge_tiles: sharded maps are not merged"); return false; }
    std::vector<std::pair<int, int>> seen((size_t)n);
    int bx0 = INT32_MAX, by0 = INT32_MAX, bx1 = INT32_MIN, by1 = INT32_MIN;
    for (int i = 0; i < n; i++) {
        if (!dev_slots[i] || ((uintptr_t)dev_slots[i] & 15)) { set_error("merge_tiles: a slot image is null or not 16-byte aligned"); return false; }
        if (std::abs((long long)xy[2 * i]) > (1 << 28) || std::abs((long long)xy[2 * i + 1]) > (1 << 28)) { set_error("merge_tiles: tile coordinate out of range"); return false; }
        seen[i] = { xy[2 * i + 1], xy[2 * i] };
        bx0 = std::min(bx0, xy[2 * i]); bx1 = std::max(bx1, xy[2 * i] + 1); by0 = std::min(by0, xy[2 * i + 1]); by1 = std::max(by1, xy[2 * i + 1] + 1);
    }
    std::sort(seen.begin(), seen.end());
    if (std::adjacent_find(seen.begin(), seen.end()) != seen.end()) { set_error("merge_tiles: a tile coordinate is given twice"); return false; }
    if (!set_device() || !drain()) return false;
    if (n == 0) return true;
    grow_to(bx0, by0, bx1, by1);
    std::vector<MergeItem> items((size_t)n);
    for (int i = 0; i < n; i++) items[i] = MergeItem{ xy[2 * i], xy[2 * i + 1], dev_slots[i], wlb16 ? wlb16 + 16 * (size_t)i : nullptr };
    return merge_items(items);
}

bool FusionMap::tile_bounds(int ix, int iy, float wlb16[16])
{
    std::lock_guard<std::mutex> l(mu_); (void)drain();
    Tile* t = store_.find(ix, iy);
    if (!t || t->fresh) return false;
    std::memcpy(wlb16, t->wlb, sizeof(t->wlb));
    return true;
}

// ------------------------------------------------------------------ state file (state_file.hpp)
bool FusionMap::save_state(const char* path)
{
    namespace sf = statefile;
    if (!init_ok_ || !path) { set_error("save_state: no device or no path"); return false; }
    wait_worker_idle();
    std::lock_guard<std::mutex> l(mu_);
    if (!valid_) { set_error("save_state: the map is not prepared"); return false; }
    if (opt_.shard_count > 1) { set_error("save_state: a sharded map holds a part of the mosaic only"); return false; }
    if (!set_device() || !drain() || !settle()) return false;
    HIP_OK(sync_all());
    std::vector<std::pair<std::pair<int, int>, Tile*>> held;
    store_.for_each([&](int ix, int iy, Tile& t) { if (!t.fresh) held.push_back({ { iy, ix }, &t }); });
    std::sort(held.begin(), held.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
    sf::StateHeader h{};
    std::memcpy(h.magic, sf::kMagic, sizeof(h.magic));
    h.version = sf::kVersion; h.header_bytes = sizeof(h);
    h.map_type = single_band_ ? sf::kTypeSingleBand : sf::kTypeMultiBand; h.pyramid_type = pyramid_type(); h.band_number = band_num_; h.weight_type = opt_.weight_type;
    h.slot_bytes = lay_.slot_bytes; h.n_tiles = held.size();
    std::memcpy(h.plane, plane_.t, 24); std::memcpy(h.plane + 3, plane_.q, 32); std::memcpy(h.cam, &cam_, 48);
    std::memcpy(h.min0, min0_, 24); std::memcpy(h.min, min_, 24); std::memcpy(h.max, max_, 24);
    h.ele_size = ele_size_; h.length_pixel = length_pixel_; h.w = w_; h.h = h_; h.off_x = off_x_; h.off_y = off_y_;
    if (sf::slot_bytes_of(h.map_type, h.pyramid_type, h.band_number) != h.slot_bytes) { set_error("save_state: the slot layout is not the state file's"); return false; }
    // the gaps between the levels of a slot (each level starts on 256 bytes) hold whatever the allocation held: written as zeros
    std::vector<std::pair<size_t, size_t>> gaps;
    if (!single_band_) {
        const size_t es = lay_.f32 ? 4 : 2;
        for (int i = 0; i < lay_.nlev; i++) {
            const size_t n = (size_t)(kElePixels >> i) * (kElePixels >> i);
            const size_t lap_end = lay_.lap_off[i] + n * 3 * es, w_end = lay_.w_off[i] + n * 4;
            const size_t lap_next = i + 1 < lay_.nlev ? lay_.lap_off[i + 1] : lay_.w_off[0], w_next = i + 1 < lay_.nlev ? lay_.w_off[i + 1] : lay_.slot_bytes;
            if (lap_next > lap_end) gaps.push_back({ lap_end, lap_next - lap_end });
            if (w_next > w_end) gaps.push_back({ w_end, w_next - w_end });
        }
    }
    const std::string tmp = std::string(path) + ".part";
    std::FILE* f = std::fopen(tmp.c_str(), "wb");
    if (!f) { set_error("save_state: cannot create " + tmp); return false; }
    bool ok = std::fwrite(&h, sizeof(h), 1, f) == 1;
    const size_t batch = std::max<size_t>(1, ((size_t)64 << 20) / lay_.slot_bytes);
    std::vector<uint8_t> host(std::min(batch, std::max<size_t>(held.size(), 1)) * lay_.slot_bytes);
    for (size_t o = 0; ok && o < held.size(); o += batch) {
        const size_t nb = std::min(batch, held.size() - o);
        std::vector<OutPiece> pieces(nb);
        for (size_t k = 0; k < nb; k++) pieces[k] = OutPiece{ host.data() + k * lay_.slot_bytes, held[o + k].second->base, lay_.slot_bytes };
        ok = download(pieces);                   // through the pinned staging ring
        for (size_t k = 0; ok && k < nb; k++) {
            sf::TileHead th{};
            th.ix = held[o + k].first.second; th.iy = held[o + k].first.first;
            std::memcpy(th.wlb, held[o + k].second->wlb, sizeof(th.wlb));
            sf::sanitize(th);
            uint8_t* img = host.data() + k * lay_.slot_bytes;
            for (auto& g : gaps) std::memset(img + g.first, 0, g.second);
            ok = std::fwrite(&th, sizeof(th), 1, f) == 1 && std::fwrite(img, lay_.slot_bytes, 1, f) == 1;
            if (!ok) set_error("save_state: write failed");
        }
    }
    if (std::fclose(f) != 0 && ok) { ok = false; set_error("save_state: write failed"); }
    if (ok && std::rename(tmp.c_str(), path) != 0) { ok = false; set_error("save_state: cannot move the file into place"); }
    if (!ok) std::remove(tmp.c_str());           // no file is left behind
    return ok;
}

// the records of a validated file merged in bounded batches: file -> pinned staging -> HBM -> merge_items
bool FusionMap::merge_records(std::FILE* f, const void* header, const void* heads_v)
{
    namespace sf = statefile;
    const sf::StateHeader& h = *(const sf::StateHeader*)header;
    const std::vector<sf::TileHead>& heads = *(const std::vector<sf::TileHead>*)heads_v;
    if (heads.empty()) return true;
    if (!out_ring_init()) return false;
    const size_t batch = std::max<size_t>(1, kOutSlot / lay_.slot_bytes);
    if (!merge_stage_.reserve(std::min(batch, heads.size()) * lay_.slot_bytes)) return false;
    for (size_t o = 0; o < heads.size(); o += batch) {
        const size_t nb = std::min(batch, heads.size() - o);
        for (size_t k = 0; k < nb; k++)
            if (!sf::read_slot(f, h, o + k, out_pin_[0] + k * lay_.slot_bytes)) { set_error("state file: cannot read a tile record"); return false; }
        HIP_OK(hipMemcpyAsync(merge_stage_.p, out_pin_[0], nb * lay_.slot_bytes, hipMemcpyHostToDevice, stream_));
        std::vector<MergeItem> items(nb);
        for (size_t k = 0; k < nb; k++) items[k] = MergeItem{ heads[o + k].ix, heads[o + k].iy, (const char*)merge_stage_.p + k * lay_.slot_bytes, heads[o + k].wlb };
        if (!merge_items(items)) return false;   // (ends with the stream idle: the staging buffers are free for the next batch)
    }
    return true;
}

bool FusionMap::merge_state(const char* path)
{
    namespace sf = statefile;
    if (!init_ok_) { set_error("merge_state: no device"); return false; }
    sf::StateHeader h; std::vector<sf::TileHead> heads; std::string why;
    std::FILE* f = path ? std::fopen(path, "rb") : nullptr;
    if (!f) { set_error("merge_state: cannot open the state file"); return false; }
    struct Close { std::FILE* f; ~Close() { std::fclose(f); } } close{ f };
    if (!sf::scan(f, h, &heads, why)) { set_error("merge_state: " + why); return false; }
    wait_worker_idle();
    std::lock_guard<std::mutex> l(mu_);
    if (!valid_) { set_error("merge_state: the map is not prepared"); return false; }
    if (opt_.shard_count > 1) { set_error("merge_state: sharded maps are not merged"); return false; }
    if (!merge_compatible("merge_state", h.map_type == sf::kTypeSingleBand, h.pyramid_type, h.band_number, h.weight_type, h.plane, h.cam, h.min0, h.ele_size, h.length_pixel)) return false;
    if (!set_device() || !drain()) return false;
    grow_to(h.off_x, h.off_y, h.off_x + h.w, h.off_y + h.h);
    return merge_records(f, &h, &heads);
}

// "prepare from the file": the old content goes as in a second prepare(), plane, camera and grid are the file's verbatim
bool FusionMap::load_state(const char* path)
{
    namespace sf = statefile;
    if (!init_ok_) { set_error("load_state: no device"); return false; }
    sf::StateHeader h; std::vector<sf::TileHead> heads; std::string why;
    std::FILE* f = path ? std::fopen(path, "rb") : nullptr;
    if (!f) { set_error("load_state: cannot open the state file"); return false; }
    struct Close { std::FILE* f; ~Close() { std::fclose(f); } } close{ f };
    if (!sf::scan(f, h, &heads, why)) { set_error("load_state: " + why); return false; }
    if (opt_.shard_count > 1) { set_error("load_state: a sharded map holds a part of the mosaic only"); return false; }
    if ((h.map_type == sf::kTypeSingleBand) != single_band_ || h.pyramid_type != pyramid_type() || h.band_number != band_num_ || h.weight_type != opt_.weight_type) {
        set_error("load_state: the map's options (type, pyramid type, band number, weight type) are not the file's");
        return false;
    }
    {
        std::unique_lock<std::mutex> q(qmu_);
        for (auto& fr : queue_) if (fr.slot >= 0) slots_[fr.slot].queued = false;
        queue_.clear();
        idle_cv_.wait(q, [this] { return !worker_busy_; });
    }
    std::lock_guard<std::mutex> l(mu_);
    if (!set_device()) return false;
    if (valid_) (void)drain();
    for (auto& p : pending_) release_slot(p.f);
    pending_.clear();
    HIP_OK(sync_all());
    store_.clear();
    // the file does not carry an input camera (the map is in the output camera's geometry): the caller sets it again
    und_set_ = false; und_table_.release(); und_uncovered_ = 0;
    plane_ = pose_from7(h.plane); plane_inv_ = inverse(plane_);
    cam_ = Camera{ h.cam[0], h.cam[1], h.cam[2], h.cam[3], h.cam[4], h.cam[5], 1. / h.cam[2], 1. / h.cam[3] };
    length_pixel_ = h.length_pixel; length_pixel_inv_ = 1. / h.length_pixel;
    ele_size_ = h.ele_size; ele_size_inv_ = 1. / h.ele_size;
    std::memcpy(min_, h.min, 24); std::memcpy(max_, h.max, 24); std::memcpy(min0_, h.min0, 24);
    w_ = h.w; h_ = h.h; off_x_ = h.off_x; off_y_ = h.off_y;
    valid_ = true;
    return merge_records(f, &h, &heads);
}

}  // namespace pf
