// map_support.hpp -- what the map engine (fusion_map.hpp) is made of besides the map itself: error text, the tile store, the owners of
// GPU resources (DevBuf, OutRing, KernelProfiler: each frees what it holds in its destructor), section names and roctx ranges.
// map_support.cpp, but for OutRing (map_output.cpp).
#pragma once
#include "kernels.hpp"
#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

namespace pf {

void set_error(const std::string& msg);
const char* last_error();

// spatial-hash owner of a tile; cells of shard_block tiles
int tile_owner(int shard_count, int shard_block, int ix, int iy);

// ---- tile store: spatial hash (ix,iy) -> slot in an HBM slab pool ----------
// replaces the dense vector<SPtr<Ele>> + spreadMap re-layout (.h:91, .cpp:561-604)
struct Tile {
    char* base = nullptr;   // slot base in HBM
    bool  fresh = true;     // pyr_laplace[i].empty() (.cpp:498): first write copies unconditionally
    bool  changed = false;  // Ele::Ischanged
    // A lower bound of every weight stored in this tile, all levels (render_frame's cull): each keyframe whose canvas holds the
    // tile raises it to the smallest weight that keyframe can have anywhere in the cell's pyramid support.  <= 0: nothing known.
    // Per cell of the cull, row-major: 4 x 4 cells of 64 x 64 pixels (PF_CULL_SUB=2: 2 x 2 quadrants in the first four)
    float wlb[16] = { -1.f, -1.f, -1.f, -1.f, -1.f, -1.f, -1.f, -1.f, -1.f, -1.f, -1.f, -1.f, -1.f, -1.f, -1.f, -1.f };
};

class TileStore {
public:
    ~TileStore() { clear(); }
    void  configure(size_t slot_bytes) { slot_bytes_ = slot_bytes; }
    // (find and get_or_create are called once per tile of every keyframe's canvas: inline, so that the render path's calls stay what they
    // were when the store lived in its translation unit)
    Tile* find(int ix, int iy)
    {
        auto it = map_.find(key(ix, iy));
        return it == map_.end() ? nullptr : &it->second;
    }
    Tile* get_or_create(int ix, int iy)           // nullptr on HBM exhaustion
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
    bool  reserve(size_t n_tiles, std::vector<std::pair<char*, size_t>>* fresh = nullptr);   // slabs for n more tiles now
    void  clear();
    size_t size() const { return map_.size(); }
    template <class F> void for_each(F f) { for (auto& kv : map_) f((int)(int32_t)(kv.first >> 32), (int)(int32_t)(kv.first & 0xffffffffu), kv.second); }
#if PF_EXPERIMENTS
    // test hook (pf_debug_tile_store): from now on get_or_create opens slabs of slab_slots tiles (0: the default size; > 0 also closes the
    // slab in progress, so that the next new tile opens slab 0), and of the slabs asked for from now on those numbered fail_from ..
    // fail_from + fail_count - 1 are asked of hipMalloc at 2^60 bytes, which it refuses as it refuses a request the device cannot meet
    void debug_limits(int slab_slots, int fail_from, int fail_count)
    {
        dbg_slab_ = slab_slots > 0 ? (size_t)slab_slots : 0; dbg_no_ = 0; dbg_from_ = fail_from; dbg_count_ = fail_count;
        if (dbg_slab_ && !chunks_.empty()) next_in_chunk_ = chunks_[cur_].slots;
    }
#endif
private:
    static uint64_t key(int ix, int iy) { return ((uint64_t)(uint32_t)ix << 32) | (uint32_t)iy; }
    std::unordered_map<uint64_t, Tile> map_;
    struct Chunk { char* p; size_t slots; };
    std::vector<Chunk> chunks_;                   // chunks_[cur_] is being filled, later ones are reserved ahead
    size_t slot_bytes_ = 0, cur_ = 0, next_in_chunk_ = 0;
    bool   add_chunk(size_t slots);
    size_t slab_slots() const;                    // slabs of ~256 MiB: few hipMallocs, tiles of one neighbourhood stay close in HBM
#if PF_EXPERIMENTS
    size_t dbg_slab_ = 0; long dbg_no_ = 0, dbg_from_ = 0, dbg_count_ = 0;
#endif
};

// A grow-only device buffer that frees itself.  Moved, never copied (the input camera's table is built aside and moved into place)
struct DevBuf {
    void*  p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    ~DevBuf() { release(); }
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; } return *this; }
    bool   reserve(size_t bytes);     // grow-only; caller must have synchronised users
    void   release();
};

// ---- output ring (map_output.cpp) ----
// Results leave HBM through a ring of two pinned staging slots: the device-to-host copy of piece k+1 (its own copy stream) runs while
// the host moves piece k from its slot into the caller's (pageable) buffer on a few threads.  A blocking hipMemcpy into
// pageable memory -- what rounds 1-5 did -- moves 12 GB/s on the boxes used; a caller who hands over pinned memory
// (pf_host_alloc) gets the copy straight into it.  Made by the first call that needs it: a map that never reads back pins nothing.
struct OutPiece { void* dst; const void* src; size_t bytes; };      // host destination, device source
class OutRing {
public:
    static constexpr size_t kSlot = (size_t)32 << 20;
    OutRing() = default;
    ~OutRing();
    OutRing(const OutRing&) = delete;
    OutRing& operator=(const OutRing&) = delete;
    // `pieces` = (host destination, device source, bytes) in the order they become ready; everything they read has been queued on
    // `stream` before the call.  Pieces are cut to the slot size.
    bool download(hipStream_t stream, const std::vector<OutPiece>& pieces);
    uint8_t* stage();           // slot 0 as kSlot bytes of pinned staging for the way INTO HBM (the state file's records); nullptr: no ring
private:
    uint8_t*    pin_[2]{};
    hipEvent_t  copied_[2]{}, ready_ = nullptr;
    hipStream_t copy_stream_ = nullptr;
    int         threads_ = 1;
    bool        ok_ = false;
    bool init();
};

// ---- kernel-event profiler ----
// Brackets launches with event pairs and sums what they took per kernel id (kernels.hpp, K_COUNT).  mode: 0 off, 1 every kernel,
// 2 + k only kernel k; bits 8 and up: every n-th launch of a kernel only.
class KernelProfiler {
public:
    KernelProfiler() = default;
    ~KernelProfiler();
    KernelProfiler(const KernelProfiler&) = delete;
    KernelProfiler& operator=(const KernelProfiler&) = delete;
    void set_mode(int mode) { mode_ = mode; }
    bool would(int id) const;                                      // will the next begin(id) bracket its launch with events?
    // bytes: SURVEY 8d's algorithmic bytes of the launch for EVERY tile of the canvas; bytes_run (< 0: the same): those of the part of the
    // canvas its blocks actually process (the cull / a shard leave blocks out) -- the numerator of bench.py's roofline.frac
    void begin(int id, double bytes, hipStream_t stream, double bytes_run);
    bool end();                 // true: more than 4096 pairs wait -- the owner synchronises its streams and calls harvest()
    double* last_bytes_run();   // the record of the launch end() just closed, if it was bracketed (else nullptr): its bytes_run may be corrected
    void harvest();             // every pair recorded so far has completed (the caller has synchronised)
    int  read(int cap, const char** names, double* ms, long long* launches, double* bytes, double* bytes_run) const;
    void reset();
private:
    struct Rec { int id; hipEvent_t a, b; double bytes, bytes_run; };
    int mode_ = 0; bool on_ = false;
    unsigned tick_[K_COUNT]{};
    std::vector<Rec> pending_;
    std::vector<hipEvent_t> pool_;
    double ms_[K_COUNT]{}; long long n_[K_COUNT]{}; double bytes_[K_COUNT]{}, bytes_run_[K_COUNT]{};
    Rec cur_{};
    hipStream_t stream_ = nullptr;
};

// Named host sections, after pi::Timer (PIL/src/base/time/Timer.h:43-85: enter / leave, calls, min / max / mean per
// section) with the reference's own section names (MultiBandMap2DCPU.cpp:476,555,563,602,628-630,722,742); each section is
// also a roctx range when PF_ROCTX=1 (rocprofv3 --marker-trace shows them next to the kernels).
enum SectionId { T_FEED = 0, T_RENDER, T_APPLY, T_SPREAD, T_UPDATE_TEXTURE, T_SAVE, T_COUNT };
const char* section_name(int id);
struct SectionRec { long long n_calls = 0; double min_t = 0, max_t = 0, total_t = 0; };
void roctx_push(const char* name);
void roctx_pop();

}  // namespace pf
