// map_merge.cpp -- map merge and the state file (fusion_map.hpp, merge.hpp, state_file.hpp).
#include "fusion_map.hpp"
#include "map_internal.hpp"
#include "state_file.hpp"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

namespace pf {

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
    Drained l(*this);
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
        ok = out_ring_.download(stream_, pieces);                  // through the pinned staging ring
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
    uint8_t* const pin = out_ring_.stage();
    if (!pin) return false;
    const size_t batch = std::max<size_t>(1, OutRing::kSlot / lay_.slot_bytes);
    if (!merge_stage_.reserve(std::min(batch, heads.size()) * lay_.slot_bytes)) return false;
    for (size_t o = 0; o < heads.size(); o += batch) {
        const size_t nb = std::min(batch, heads.size() - o);
        for (size_t k = 0; k < nb; k++)
            if (!sf::read_slot(f, h, o + k, pin + k * lay_.slot_bytes)) { set_error("state file: cannot read a tile record"); return false; }
        HIP_OK(hipMemcpyAsync(merge_stage_.p, pin, nb * lay_.slot_bytes, hipMemcpyHostToDevice, stream_));
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
