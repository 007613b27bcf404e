// map_output.cpp -- the way out of the map (fusion_map.hpp): tile access, seam-exchange support, the pinned output ring, blend.
#include "fusion_map.hpp"
#include "map_internal.hpp"
#include "env.hpp"
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <thread>

namespace pf {

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
    Drained l(*this);
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
    Drained l(*this);
    int n = 0;
    store_.for_each([&](int, int, Tile& t) { if (!t.fresh) n++; });
    return n;
}

int FusionMap::tile_coords(int* xy, int cap)
{
    Drained l(*this);
    std::vector<std::pair<int, int>> v;
    store_.for_each([&](int ix, int iy, Tile& t) { if (!t.fresh) v.push_back({ iy, ix }); });
    std::sort(v.begin(), v.end());
    for (size_t i = 0; i < v.size() && (int)i < cap; i++) { xy[2 * i] = v[i].second; xy[2 * i + 1] = v[i].first; }
    return (int)v.size();
}

bool FusionMap::get_tile_bgra(int ix, int iy, uint8_t* bgra)
{
    Drained l(*this);
    if (!init_ok_ || !single_band_ || !set_device()) return false;
    Tile* t = store_.find(ix, iy);
    if (!t || t->fresh) return false;
    HIP_OK(sync_all());
    HIP_OK(hipMemcpy(bgra, t->base, (size_t)kElePixels * kElePixels * 4, hipMemcpyDeviceToHost));
    return true;
}

bool FusionMap::get_tile_level(int ix, int iy, int level, void* lap, float* w)
{
    Drained l(*this);
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
    Drained l(*this);
    if (!init_ok_ || !set_device()) return false;
    Tile* t = store_.find(ix, iy);
    if (!t || t->fresh) return false;
    launch_halo_pack(stream_, lay_, t->base, dx, dy, dev_out);
    HIP_OK(sync_all());
    return true;
}

bool FusionMap::tile_export(int ix, int iy, void* dev_out)
{
    Drained l(*this);
    if (!init_ok_ || !set_device()) return false;
    Tile* t = store_.find(ix, iy);
    if (!t || t->fresh) return false;
    HIP_OK(hipMemcpyAsync(dev_out, t->base, lay_.slot_bytes, hipMemcpyDeviceToDevice, stream_));
    HIP_OK(sync_all());
    return true;
}

bool FusionMap::tile_import(int ix, int iy, const void* dev_in)
{
    Drained l(*this);
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
    Drained l(*this);
    out.clear();
    store_.for_each([&](int ix, int iy, Tile& t) { if (!t.fresh) out.push_back({ ix, iy, t.changed ? 1 : 0 }); });
    std::sort(out.begin(), out.end(), [](const TileRec& a, const TileRec& b) { return a.iy != b.iy ? a.iy < b.iy : a.ix < b.ix; });
}

// every strip set of one exchange: one descriptor upload, one launch, no sync (the caller orders its transport after stream_)
bool FusionMap::pack_strips(const std::vector<StripReq>& reqs, void* dev_out)
{
    Drained l(*this);
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
    Drained l(*this);
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
    Drained l(*this);
    if (!init_ok_ || !set_device() || single_band_) return false;
    if (!blend_batch(tiles, halo9, nullptr, bgr)) return false;
    for (auto& t : tiles) { Tile* q = store_.find(t.first, t.second); if (q) q->changed = false; }
    return true;
}

// ------------------------------------------------------------------ output side
// the output ring (OutRing, map_support.hpp)
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

bool OutRing::init()
{
    if (ok_) return true;
    // (a call that failed half way is finished by the next one: every piece is made once)
    for (int i = 0; i < 2; i++) {
        if (!pin_[i]) HIP_OK(hipHostMalloc((void**)&pin_[i], kSlot, hipHostMallocDefault));
        if (!copied_[i]) HIP_OK(hipEventCreateWithFlags(&copied_[i], hipEventDisableTiming));
    }
    if (!ready_) HIP_OK(hipEventCreateWithFlags(&ready_, hipEventDisableTiming));
    if (!copy_stream_) HIP_OK(hipStreamCreateWithFlags(&copy_stream_, hipStreamNonBlocking));
    ok_ = true;
    const unsigned hc = std::thread::hardware_concurrency();
    threads_ = std::getenv("PF_COPY_THREADS") ? std::atoi(std::getenv("PF_COPY_THREADS")) : (int)std::min(8u, std::max(1u, hc / 2));
    return true;
}

OutRing::~OutRing()
{
    for (int i = 0; i < 2; i++) { if (pin_[i]) (void)hipHostFree(pin_[i]); if (copied_[i]) (void)hipEventDestroy(copied_[i]); }
    if (ready_) (void)hipEventDestroy(ready_);
    if (copy_stream_) (void)hipStreamDestroy(copy_stream_);
}

uint8_t* OutRing::stage() { return init() ? pin_[0] : nullptr; }

bool OutRing::download(hipStream_t stream, const std::vector<OutPiece>& pieces)
{
    if (pieces.empty()) return true;
    if (!init()) return false;
    HIP_OK(hipEventRecord(ready_, stream));
    HIP_OK(hipStreamWaitEvent(copy_stream_, ready_, 0));
    struct Part { char* dst; const char* src; size_t n; bool direct; };
    std::vector<Part> parts;
    for (auto& pc : pieces) {
        const bool direct = is_pinned_host(pc.dst);
        for (size_t o = 0; o < pc.bytes; o += kSlot) parts.push_back({ (char*)pc.dst + o, (const char*)pc.src + o, std::min(kSlot, pc.bytes - o), direct });
    }
    int k = 0;                                  // staged parts issued so far
    long prev = -1; int prev_slot = 0;          // staged part whose bytes still sit in its slot
    auto drain = [&]() -> bool {
        if (prev < 0) return true;
        HIP_OK(hipEventSynchronize(copied_[prev_slot]));
        copy_threads(parts[prev].dst, pin_[prev_slot], parts[prev].n, threads_);
        prev = -1;
        return true;
    };
    for (size_t i = 0; i < parts.size(); i++) {
        const Part& pt = parts[i];
        if (pt.direct) { HIP_OK(hipMemcpyAsync(pt.dst, pt.src, pt.n, hipMemcpyDeviceToHost, copy_stream_)); continue; }
        const int slot = k++ & 1;               // its previous tenant (two staged parts ago) has been drained: drain() runs once per staged part
        HIP_OK(hipMemcpyAsync(pin_[slot], pt.src, pt.n, hipMemcpyDeviceToHost, copy_stream_));
        HIP_OK(hipEventRecord(copied_[slot], copy_stream_));
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
        if (!out_ring_.download(stream_, pieces)) return false;      // also orders the next launch's job upload and result buffers after this one's readers
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

bool FusionMap::blend_tile(int ix, int iy, void* raw, uint8_t* bgr, const void* const* halo)
{
    if (single_band_) {          // the Map2DCPU tile is displayable as is (glTexImage2D GL_BGRA, Map2DCPU.cpp:497-503)
        std::vector<uint8_t> px((size_t)kElePixels * kElePixels * 4);
        if (!get_tile_bgra(ix, iy, px.data())) return false;
        if (raw) std::memcpy(raw, px.data(), px.size());
        if (bgr) bgra_to_bgr(px.data(), bgr, (size_t)kElePixels * kElePixels);
        return true;
    }
    Drained l(*this);
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
    Drained l(*this);
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
    Drained l(*this);
    if (!init_ok_ || !set_device()) return false;
    TileJpeg tj{ quality, out, cap, offsets };
    return blend_batch(tiles, nullptr, nullptr, nullptr, &tj);
}

// the draw() loop's texture refresh (.cpp:705-742) without GL; level > 0: the same tiles as views of that level, (256 >> level)^2 x 3 bytes each
int FusionMap::blend_changed(int* xy, uint8_t* bgr, int cap, int level)
{
    if (!level_ok("pf_blend_changed_level", level)) return 0;
    Drained l(*this);
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

}  // namespace pf
