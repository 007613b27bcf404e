// map_support.cpp -- under the map engine (map_support.hpp): error text, tile owner, section timers and roctx ranges, the tile
// store, DevBuf, the kernel-event profiler.
#include "fusion_map.hpp"
#include "map_internal.hpp"
#include "env.hpp"
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <dlfcn.h>

namespace pf {

static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; std::fprintf(stderr, "pifusion: %s\n", msg.c_str()); }
const char* last_error() { return g_err.c_str(); }

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

// ---------------------------------------------------------------- profile
KernelProfiler::~KernelProfiler()
{
    for (auto& r : pending_) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    for (auto e : pool_) (void)hipEventDestroy(e);
}

bool KernelProfiler::would(int id) const
{
    const int what = mode_ & 0xff, every = mode_ >> 8;
    return (what == 1 || what == 2 + id) && (every <= 1 || tick_[id] % every == 0);
}

void KernelProfiler::begin(int id, double bytes, hipStream_t stream, double bytes_run)
{
    stream_ = stream;
    const int what = mode_ & 0xff, every = mode_ >> 8;
    on_ = what == 1 || what == 2 + id;                  // mode 2+k: only kernel k
    // event pairs are not free (each is a marker packet between two launches): optionally time every n-th launch only
    if (on_ && every > 1) on_ = (tick_[id]++ % every) == 0;
    if (!on_) return;
    auto get = [&]() { hipEvent_t e; if (!pool_.empty()) { e = pool_.back(); pool_.pop_back(); } else (void)hipEventCreate(&e); return e; };
    cur_ = { id, get(), get(), bytes, bytes_run < 0 ? bytes : bytes_run };
    (void)hipEventRecord(cur_.a, stream_);
}

bool KernelProfiler::end()
{
    if (!on_) return false;
    (void)hipEventRecord(cur_.b, stream_);
    pending_.push_back(cur_);
    return pending_.size() > 4096;
}

double* KernelProfiler::last_bytes_run() { return on_ && !pending_.empty() ? &pending_.back().bytes_run : nullptr; }

void KernelProfiler::harvest()
{
    for (auto& r : pending_) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) { ms_[r.id] += ms; n_[r.id]++; bytes_[r.id] += r.bytes; bytes_run_[r.id] += r.bytes_run; }
        pool_.push_back(r.a); pool_.push_back(r.b);
    }
    pending_.clear();
}

int KernelProfiler::read(int cap, const char** names, double* ms, long long* launches, double* bytes, double* bytes_run) const
{
    int n = 0;
    for (int i = 0; i < K_COUNT && n < cap; i++, n++) {
        names[n] = kernel_name(i); ms[n] = ms_[i]; launches[n] = n_[i]; bytes[n] = bytes_[i];
        if (bytes_run) bytes_run[n] = bytes_run_[i];
    }
    return n;
}

void KernelProfiler::reset() { for (int i = 0; i < K_COUNT; i++) { ms_[i] = 0; n_[i] = 0; bytes_[i] = 0; bytes_run_[i] = 0; tick_[i] = 0; } }

// (does not render what waits: switching the profiler is no reader of the map)
void FusionMap::profile_enable(int mode) { std::lock_guard<std::mutex> l(mu_); prof_.set_mode(mode); }

int FusionMap::profile_read(int cap, const char** names, double* ms, long long* launches, double* bytes, double* bytes_run)
{
    Drained l(*this);
    (void)hipSetDevice(device_);
    (void)sync_all();
    prof_.harvest();
    return prof_.read(cap, names, ms, launches, bytes, bytes_run);
}

void FusionMap::profile_reset()
{
    Drained l(*this);
    (void)hipSetDevice(device_);
    (void)sync_all();
    prof_.harvest();
    prof_.reset();
}

}  // namespace pf
