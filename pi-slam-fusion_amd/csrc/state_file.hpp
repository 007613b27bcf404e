// state_file.hpp -- the map state file: format, writer pieces and the validating parser.  Pure host code, no HIP: the engine
// (map_merge.cpp: save_state / load_state / merge_state), pf_state_info and tests/cpp/state_file_check.cpp include it.
//
// Little-endian, a pure function of the map's state (no time stamp, no pointer, no padding left unset):
//   header   256 bytes (StateHeader)
//   records  n_tiles of them, sorted by (iy, ix) like FusionMap::list_tiles, each
//            int32 ix, iy (stable tile coordinates) | float wlb[16] (the tile's cull bounds) | the slot image, slot_bytes bytes
//
// The parser checks everything it can before the map is touched: magic, version, the options' ranges, that slot_bytes is what the
// layout of that type and band count gives, that the file is exactly header + n_tiles records long, finite geometry, coordinates inside the
// header's grid, sorted and therefore unique.  A wlb that is not finite reads as -1 (nothing known).  PIXEL CONTENT IS NOT CHECKED: the Laplacians and weights
// of a record are as trusted as a slot handed to pf_tile_import -- a file from elsewhere can hold any bits there, and the map will hold them.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace pf {
namespace statefile {

static_assert(__BYTE_ORDER__ == __ORDER_LITTLE_ENDIAN__, "the state file is little-endian and written from memory");

constexpr char     kMagic[8] = { 'P', 'I', 'F', 'U', 'M', 'A', 'P', '\n' };
constexpr uint32_t kVersion = 1;
constexpr int      kTilePixels = 256, kMaxBands = 8;
// the codes of include/pifusion.h (PF_TYPE_CPU, PF_TYPE_MULTIBAND_CPU, PF_8UC4, PF_16SC3, PF_32FC3), restated: this header stands alone
constexpr int32_t  kTypeSingleBand = 1, kTypeMultiBand = 3, k8UC4 = 24, k16SC3 = 19, k32FC3 = 21;

struct StateHeader {
    char     magic[8];
    uint32_t version, header_bytes;
    int32_t  map_type, pyramid_type, band_number, weight_type;
    uint64_t slot_bytes, n_tiles;
    double   plane[7], cam[6], min0[3], min[3], max[3], ele_size, length_pixel;
    int32_t  w, h, off_x, off_y;
};
static_assert(sizeof(StateHeader) == 256, "StateHeader is the file's first 256 bytes");

struct TileHead { int32_t ix, iy; float wlb[16]; };
static_assert(sizeof(TileHead) == 72, "TileHead is a record's first 72 bytes");

// TileLayout::slot_bytes of make_layout (kernels.hip), and the single-band slot; 0: no such map
inline uint64_t slot_bytes_of(int32_t map_type, int32_t pyramid_type, int32_t band_number)
{
    if (map_type == kTypeSingleBand) return pyramid_type == k8UC4 && band_number == 0 ? (uint64_t)kTilePixels * kTilePixels * 4 : 0;
    if (map_type != kTypeMultiBand || (pyramid_type != k16SC3 && pyramid_type != k32FC3) || band_number < 0 || band_number > kMaxBands) return 0;
    const uint64_t es = pyramid_type == k32FC3 ? 4 : 2;
    uint64_t off = 0;
    for (int i = 0; i <= band_number; i++) { const uint64_t n = (uint64_t)(kTilePixels >> i) * (kTilePixels >> i); off += (n * 3 * es + 255) / 256 * 256; }
    for (int i = 0; i <= band_number; i++) { const uint64_t n = (uint64_t)(kTilePixels >> i) * (kTilePixels >> i); off += (n * 4 + 255) / 256 * 256; }
    return off;
}

inline uint64_t record_bytes(const StateHeader& h) { return sizeof(TileHead) + h.slot_bytes; }

inline bool all_finite(const double* v, int n) { for (int i = 0; i < n; i++) if (!std::isfinite(v[i])) return false; return true; }

// the header alone, against the length of the file it came from
inline bool check_header(const StateHeader& h, uint64_t file_bytes, std::string& why)
{
    if (std::memcmp(h.magic, kMagic, sizeof(kMagic)) != 0) { why = "not a map state file (magic)"; return false; }
    if (h.version != kVersion || h.header_bytes != sizeof(StateHeader)) { why = "state file of another version"; return false; }
    const uint64_t sb = slot_bytes_of(h.map_type, h.pyramid_type, h.band_number);
    if (!sb) { why = "no map of this type, pyramid type and band number"; return false; }
    if (h.slot_bytes != sb) { why = "slot_bytes is not the layout's for this type and band number"; return false; }
    const uint64_t rec = record_bytes(h), body = file_bytes - sizeof(StateHeader);
    if (file_bytes < sizeof(StateHeader) || h.n_tiles > body / rec || h.n_tiles * rec != body) { why = "file length is not header + n_tiles records"; return false; }
    if (!all_finite(h.plane, 7) || !all_finite(h.cam, 6)) { why = "plane or camera not finite"; return false; }
    if (!all_finite(h.min0, 3) || !all_finite(h.min, 3) || !all_finite(h.max, 3) || !std::isfinite(h.ele_size) || !std::isfinite(h.length_pixel)) { why = "geometry not finite"; return false; }
    if (!(h.ele_size > 0) || !(h.length_pixel > 0) || !(h.cam[0] > 0) || !(h.cam[1] > 0) || h.cam[2] == 0 || h.cam[3] == 0) { why = "geometry or camera not valid"; return false; }
    if (h.w <= 0 || h.h <= 0 || h.w > (1 << 24) || h.h > (1 << 24) || std::abs((long long)h.off_x) > (1 << 28) || std::abs((long long)h.off_y) > (1 << 28)) { why = "grid out of range"; return false; }
    return true;
}

// a record's head as the map may take it: a bound that is not finite is no bound
inline void sanitize(TileHead& t) { for (float& w : t.wlb) if (!std::isfinite(w)) w = -1.f; }

inline bool after(const TileHead& a, const TileHead& b) { return a.iy != b.iy ? a.iy > b.iy : a.ix > b.ix; }      // a strictly after b

inline bool file_size(std::FILE* f, uint64_t& n)
{
    if (fseeko(f, 0, SEEK_END) != 0) return false;
    const off_t e = ftello(f);
    if (e < 0) return false;
    n = (uint64_t)e;
    return fseeko(f, 0, SEEK_SET) == 0;
}

// Header and every record's head of an open file, validated; heads (may be null) receives them, sanitized.  The slot images are skipped.
inline bool scan(std::FILE* f, StateHeader& h, std::vector<TileHead>* heads, std::string& why)
{
    uint64_t bytes = 0;
    if (!file_size(f, bytes)) { why = "cannot size the file"; return false; }
    if (bytes < sizeof(StateHeader) || std::fread(&h, sizeof(h), 1, f) != 1) { why = "file shorter than the header"; return false; }
    if (!check_header(h, bytes, why)) return false;
    if (heads) { heads->clear(); heads->reserve((size_t)h.n_tiles); }
    TileHead prev{};
    for (uint64_t i = 0; i < h.n_tiles; i++) {
        TileHead t;
        if (fseeko(f, (off_t)(sizeof(StateHeader) + i * record_bytes(h)), SEEK_SET) != 0 || std::fread(&t, sizeof(t), 1, f) != 1) { why = "cannot read a tile record"; return false; }
        if (i && !after(t, prev)) { why = "tile records duplicate or not sorted by (iy, ix)"; return false; }
        if (t.ix < h.off_x || t.iy < h.off_y || (long long)t.ix - h.off_x >= h.w || (long long)t.iy - h.off_y >= h.h) { why = "tile outside the header's grid"; return false; }
        prev = t;
        sanitize(t);
        if (heads) heads->push_back(t);
    }
    return true;
}

inline bool scan_path(const char* path, StateHeader& h, std::vector<TileHead>* heads, std::string& why)
{
    std::FILE* f = path ? std::fopen(path, "rb") : nullptr;
    if (!f) { why = "cannot open the state file"; return false; }
    const bool ok = scan(f, h, heads, why);
    std::fclose(f);
    return ok;
}

// slot image of record i
inline bool read_slot(std::FILE* f, const StateHeader& h, uint64_t i, void* out)
{
    return fseeko(f, (off_t)(sizeof(StateHeader) + i * record_bytes(h) + sizeof(TileHead)), SEEK_SET) == 0 && std::fread(out, (size_t)h.slot_bytes, 1, f) == 1;
}

}  // namespace statefile
}  // namespace pf
