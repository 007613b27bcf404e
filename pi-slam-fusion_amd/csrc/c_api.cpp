// c_api.cpp -- extern "C" surface of libpifusion.so (include/pifusion.h).
#include "dist.hpp"
#include "jpeg_device.hpp"
#include "raw_convert.hpp"
#include "webtiles_plan.hpp"
#include "view_plan.hpp"
#include "state_file.hpp"
#include <cerrno>
#include <map>
#include <string>
#include <sys/stat.h>
#include <cstdlib>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <algorithm>
#include <vector>
#include <mutex>
#include <new>

using pf::FusionMap;

struct pf_map {
    FusionMap impl;
    pf::JpegDevice jpeg;          // pf_feed_jpeg: the decoder's device back end (staging buffers, coefficient and plane buffers)
    pf_map(int t, bool th, const pf_options& o) : impl(t, th, o) {}
    ~pf_map() { if (impl.ok() && impl.use_device()) impl.sync(); }          // the decoder's buffers go before the engine: nothing may still read them
};

// pf_jpeg_decode_device's decoder: process-wide, never torn down (the runtime may be gone at exit)
static std::mutex g_jpeg_mu;
static pf::JpegDevice* shared_jpeg(int device = 0)          // one per device: its buffers live where the first call on that device put them
{
    static pf::JpegDevice* d[64] = {};
    if (device < 0 || device >= 64) device = 0;
    if (!d[device]) d[device] = new pf::JpegDevice();
    return d[device];
}

extern "C" {

void pf_default_options(pf_options* o)
{
    o->band_number = 5; o->force_float = 0; o->high_quality_show = 1; o->weight_type = 0; o->bg_color = 0;
    o->resolution = 0; o->scale = 1; o->device = -1; o->shard_rank = 0; o->shard_count = 1; o->shard_block = 8;
    o->max_queue = 20; o->fused = 1; o->lookahead = 48;
}

int pf_options_set(pf_options* o, const char* key, const char* value)
{
    if (!o || !key || !value) return 0;
    const double v = std::atof(value);
    if (!std::strcmp(key, "MultiBandMap2DCPU.BandNumber")) o->band_number = (int)v;
    else if (!std::strcmp(key, "MultiBandMap2DCPU.ForceFloat")) o->force_float = (int)v;
    else if (!std::strcmp(key, "MultiBandMap2DCPU.HighQualityShow")) o->high_quality_show = (int)v;
    else if (!std::strcmp(key, "Map2D.WeightType")) o->weight_type = (int)v;
    else if (!std::strcmp(key, "Result.BackGroundColor")) o->bg_color = (int)v;
    else if (!std::strcmp(key, "Map2D.Resolution")) o->resolution = v;
    else if (!std::strcmp(key, "Map2D.Scale")) o->scale = v;
    else if (!std::strcmp(key, "Device")) o->device = (int)v;
    else if (!std::strcmp(key, "Shard.Rank")) o->shard_rank = (int)v;
    else if (!std::strcmp(key, "Shard.Count")) o->shard_count = (int)v;
    else if (!std::strcmp(key, "Shard.Block")) o->shard_block = (int)v;
    else if (!std::strcmp(key, "Map2D.MaxQueue")) o->max_queue = (int)v;
    else if (!std::strcmp(key, "Fused")) o->fused = (int)v;
    else if (!std::strcmp(key, "Lookahead")) o->lookahead = (int)v;
    else return 0;
    return 1;
}

pf_map* pf_create(int type, int thread, const pf_options* opt)
{
    if (type == PF_TYPE_NONE || type == PF_TYPE_RENDER) return nullptr;     // Map2D.cpp:53,56
    pf_options o;
    if (opt) o = *opt; else pf_default_options(&o);
    pf_map* m = new (std::nothrow) pf_map(type, thread != 0, o);
    if (m && !m->impl.ok()) { delete m; return nullptr; }
    return m;
}

void pf_destroy(pf_map* m) { delete m; }
const char* pf_last_error(void) { return pf::last_error(); }

int pf_prepare(pf_map* m, const double plane[7], const double cam[6], int n, const pf_image* imgs, const double* poses7)
{ return m && m->impl.prepare(plane, cam, n, imgs, poses7); }

int pf_feed(pf_map* m, const pf_image* img, const double pose[7]) { return m && m->impl.feed(img, pose, false); }
int pf_feed_device(pf_map* m, const pf_image* img, const double pose[7]) { return m && m->impl.feed(img, pose, true); }
int pf_debug_phase_stamps(unsigned long long* out, int cap_blocks) { return pf::read_phase_stamps(out, cap_blocks); }
void pf_debug_form_counts(long long out[8]) { if (out) pf::read_form_counts(out); }
void pf_debug_admission_counts(long long out[8]) { if (out) pf::read_admission_counts(out); }
long long pf_debug_compact_launches(void) { return pf::read_compact_launches(); }
int pf_debug_render_log(pf_map* m, long long* out, int cap) { return m ? m->impl.render_log(out, cap) : 0; }
void pf_set_cull(pf_map* m, int on) { if (m) m->impl.set_cull(on != 0); }
long long pf_debug_culled_cells(pf_map* m) { return m ? m->impl.culled_cells() : 0; }
double pf_debug_level0_exact_px(pf_map* m) { return m ? m->impl.level0_exact_px() : 0; }
long long pf_debug_culled_tiles(pf_map* m) { return m ? m->impl.culled_tiles() : 0; }
int pf_debug_select_counts(unsigned long long* out, int reset) { return out ? pf::read_select_counts(out, reset) : 0; }
long pf_debug_read_last_frame(pf_map* m, void* out, size_t cap) { return m ? m->impl.read_back_last_frame(out, cap) : -1; }
#if PF_EXPERIMENTS
// Experiments library only, and for that reason declared here and not in include/pifusion.h: the next accepted keyframe of m is warped with
// the frame -> canvas matrix M0 instead of the one its pose gives (one matrix per keyframe, in the order of the calls); the tile range still
// comes from the pose.  tests/test_gpu_warp_ties.py puts the warp's coordinates on cvRound's ties with it.
void pf_debug_next_homography(pf_map* m, const double M0[9]) { if (m && M0) m->impl.debug_next_homography(M0); }
// Allocation failures on request (tests/test_gpu_alloc_failure.py), injected as real refusals of hipMalloc: the request is for 2^60 bytes.
// pf_debug_tile_store: from now on the tile store opens slabs of slab_slots tiles (0: its default of about 256 MiB; > 0 also closes the slab
// in progress, so the next new tile opens the first slab counted), and of the slabs it asks for from this call on, those numbered fail_from
// .. fail_from + fail_count - 1 (0-based) fail.  pf_debug_fail_workspace: the next n calls that size the frame workspace fail.
void pf_debug_tile_store(pf_map* m, int slab_slots, int fail_from, int fail_count) { if (m) m->impl.debug_tile_store(slab_slots, fail_from, fail_count); }
void pf_debug_fail_workspace(pf_map* m, int n) { if (m) m->impl.debug_fail_workspace(n); }
#endif
unsigned pf_queue_size(pf_map* m) { return m ? m->impl.queue_size() : 0; }
int pf_sync(pf_map* m) { return m && m->impl.sync(); }
int pf_save(pf_map* m, const char* filename) { return m && filename && m->impl.save(filename); }
int pf_save_tiff(pf_map* m, const char* filename, int quality, int force_bigtiff) { return m && filename && m->impl.save_tiff(filename, quality, force_bigtiff != 0); }
int pf_save_tiff_lossless(pf_map* m, const char* filename, int masked, int force_bigtiff) { return m && filename && m->impl.save_tiff_lossless(filename, masked != 0, force_bigtiff != 0); }
int pf_save_png(pf_map* m, const char* filename, int masked) { return m && filename && m->impl.save_png(filename, masked != 0); }
int pf_save_tiff_masked(pf_map* m, const char* filename, int quality, int force_bigtiff) { return m && filename && m->impl.save_tiff_masked(filename, quality, force_bigtiff != 0); }
// pf_write_image / pf_image_info / pf_read_image: image_io.cpp (host code without a HIP dependency: also built by the sanitizer targets)
int pf_jpeg_info(const uint8_t* data, size_t len, int* rows, int* cols, int* components) { return pf::jpeg_info(data, len, rows, cols, components); }
int pf_jpeg_decode_bgr(const uint8_t* data, size_t len, uint8_t* bgr, int rows, int cols)
{ return rows > 0 && cols > 0 && pf::jpeg_decode_bgr(data, len, bgr, rows, cols, (size_t)cols * 3); }
int pf_jpeg_decode_device(const uint8_t* data, size_t len, void* dev_bgr, int rows, int cols, void* hip_stream)
{
    std::lock_guard<std::mutex> l(g_jpeg_mu);
    if (rows <= 0 || cols <= 0 || !dev_bgr) return 0;
    // the decoder of the device the destination lives on, with that device current for the call
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, dev_bgr) != hipSuccess || at.type != hipMemoryTypeDevice) { (void)hipGetLastError(); pf::set_error("pf_jpeg_decode_device: destination is not device memory"); return 0; }
    int prev = 0;
    (void)hipGetDevice(&prev);
    if (at.device != prev && hipSetDevice(at.device) != hipSuccess) { pf::set_error("pf_jpeg_decode_device: hipSetDevice failed"); return 0; }
    const int ok = shared_jpeg(at.device)->decode_to(data, len, (uint8_t*)dev_bgr, rows, cols, hip_stream);
    if (at.device != prev) (void)hipSetDevice(prev);
    return ok;
}
// pf_jpeg_encode_device's encoder: one per device, as the decoder's
static pf::JpegEncoder* shared_jpeg_encoder(int device)
{
    static pf::JpegEncoder* e[64] = {};
    if (device < 0 || device >= 64) device = 0;
    if (!e[device]) e[device] = new pf::JpegEncoder();
    return e[device];
}
int pf_jpeg_encode_device(const void* dev_bgr, int rows, int cols, size_t step, int quality, uint8_t* out, size_t cap, size_t* len, void* hip_stream)
{
    std::lock_guard<std::mutex> l(g_jpeg_mu);
    if (!dev_bgr || !len || rows <= 0 || cols <= 0) { pf::set_error("pf_jpeg_encode_device: no image, no length or a size that is not positive"); return 0; }
    if (!pf::jpeg_size_ok("pf_jpeg_encode_device", rows, cols)) return 0;
    if (step == 0) step = (size_t)cols * 3;
    if (step < (size_t)cols * 3) { pf::set_error("pf_jpeg_encode_device: step is smaller than a row"); return 0; }
    if (!out) { *len = pf::jenc::stream_bound(rows, cols); return 1; }
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, dev_bgr) != hipSuccess || at.type != hipMemoryTypeDevice) { (void)hipGetLastError(); pf::set_error("pf_jpeg_encode_device: the image is not in device memory"); return 0; }
    int prev = 0;
    (void)hipGetDevice(&prev);
    if (at.device != prev && hipSetDevice(at.device) != hipSuccess) { pf::set_error("pf_jpeg_encode_device: hipSetDevice failed"); return 0; }
    pf::JpegEncoder* e = shared_jpeg_encoder(at.device);
    size_t off[2] = { 0, 0 };
    int ok = e->encode(dev_bgr, 1, nullptr, 0, rows, cols, step, quality, off, hip_stream);
    if (ok) {
        *len = off[1];
        if (off[1] > cap) {
            pf::set_error("pf_jpeg_encode_device: the stream has " + std::to_string(off[1]) + " bytes, the buffer " + std::to_string(cap));
            (void)hipStreamSynchronize((hipStream_t)hip_stream);
            ok = 0;
        } else ok = e->fetch(out, hip_stream);
    }
    if (at.device != prev) (void)hipSetDevice(prev);
    return ok;
}
// pf_tiff_write_device's level buffers: one set per device, beside the encoder
static pf::TiffDevice* shared_tiff_device(int device)
{
    static pf::TiffDevice* t[64] = {};
    if (device < 0 || device >= 64) device = 0;
    if (!t[device]) t[device] = new pf::TiffDevice();
    return t[device];
}
int pf_tiff_write_device(const char* filename, const void* dev_bgr, int rows, int cols, size_t step, int quality, int bg, const double model_transform[16], int force_bigtiff, void* hip_stream)
{
    std::lock_guard<std::mutex> l(g_jpeg_mu);
    if (!filename || !dev_bgr || rows <= 0 || cols <= 0) { pf::set_error("pf_tiff_write_device: no name, no image or a size that is not positive"); return 0; }
    if (step == 0) step = (size_t)cols * 3;
    if (step < (size_t)cols * 3) { pf::set_error("pf_tiff_write_device: step is smaller than a row"); return 0; }
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, dev_bgr) != hipSuccess || at.type != hipMemoryTypeDevice) { (void)hipGetLastError(); pf::set_error("pf_tiff_write_device: the image is not in device memory"); return 0; }
    int prev = 0;
    (void)hipGetDevice(&prev);
    if (at.device != prev && hipSetDevice(at.device) != hipSuccess) { pf::set_error("pf_tiff_write_device: hipSetDevice failed"); return 0; }
    const int ok = shared_tiff_device(at.device)->write(filename, dev_bgr, rows, cols, step, quality, bg, model_transform, force_bigtiff != 0, *shared_jpeg_encoder(at.device), hip_stream);
    if (at.device != prev) (void)hipSetDevice(prev);
    return ok;
}
int pf_tiff_write_device_masked(const char* filename, const void* dev_bgr, int rows, int cols, size_t step, const void* dev_mask, size_t mask_step, int quality, int bg,
                                const double model_transform[16], int force_bigtiff, void* hip_stream)
{
    std::lock_guard<std::mutex> l(g_jpeg_mu);
    if (!filename || !dev_bgr || !dev_mask || rows <= 0 || cols <= 0) { pf::set_error("pf_tiff_write_device_masked: no name, no image, no mask or a size that is not positive"); return 0; }
    if (step == 0) step = (size_t)cols * 3;
    if (mask_step == 0) mask_step = (size_t)cols;
    if (step < (size_t)cols * 3 || mask_step < (size_t)cols) { pf::set_error("pf_tiff_write_device_masked: step is smaller than a row"); return 0; }
    hipPointerAttribute_t at{}, am{};
    if (hipPointerGetAttributes(&at, dev_bgr) != hipSuccess || at.type != hipMemoryTypeDevice) { (void)hipGetLastError(); pf::set_error("pf_tiff_write_device_masked: the image is not in device memory"); return 0; }
    if (hipPointerGetAttributes(&am, dev_mask) != hipSuccess || am.type != hipMemoryTypeDevice || am.device != at.device) {
        (void)hipGetLastError(); pf::set_error("pf_tiff_write_device_masked: the mask is not in device memory beside the image"); return 0;
    }
    int prev = 0;
    (void)hipGetDevice(&prev);
    if (at.device != prev && hipSetDevice(at.device) != hipSuccess) { pf::set_error("pf_tiff_write_device_masked: hipSetDevice failed"); return 0; }
    pf::TiffDevice::Mask mk;
    mk.dev_bytes = dev_mask; mk.step = mask_step;
    const int ok = shared_tiff_device(at.device)->write(filename, dev_bgr, rows, cols, step, quality, bg, model_transform, force_bigtiff != 0, *shared_jpeg_encoder(at.device), hip_stream, &mk);
    if (at.device != prev) (void)hipSetDevice(prev);
    return ok;
}
// pf_deflate_tiles_device's and pf_tiff_write_device_lossless's encoder: one per device, as the JPEG one
static pf::DeflateEncoder* shared_deflate_encoder(int device)
{
    static pf::DeflateEncoder* e[64] = {};
    if (device < 0 || device >= 64) device = 0;
    if (!e[device]) e[device] = new pf::DeflateEncoder();
    return e[device];
}
int pf_deflate_tiles_device(const void* dev_base, int n, const long long* byte_offsets, size_t step, uint8_t* out, size_t cap, size_t* offsets, void* hip_stream)
{
    std::lock_guard<std::mutex> l(g_jpeg_mu);
    if (!dev_base || n <= 0 || !byte_offsets || !offsets) { pf::set_error("pf_deflate_tiles_device: no image, no tiles or no room for the offsets"); return 0; }
    if (step == 0) step = (size_t)pf::dfl::kRowBytes;
    if (step < (size_t)pf::dfl::kRowBytes) { pf::set_error("pf_deflate_tiles_device: step is smaller than a row"); return 0; }
    for (int i = 0; i < n; i++) if (byte_offsets[i] < 0) { pf::set_error("pf_deflate_tiles_device: a tile begins in front of the allocation"); return 0; }
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, dev_base) != hipSuccess || at.type != hipMemoryTypeDevice) { (void)hipGetLastError(); pf::set_error("pf_deflate_tiles_device: the image is not in device memory"); return 0; }
    int prev = 0;
    (void)hipGetDevice(&prev);
    if (at.device != prev && hipSetDevice(at.device) != hipSuccess) { pf::set_error("pf_deflate_tiles_device: hipSetDevice failed"); return 0; }
    pf::DeflateEncoder* e = shared_deflate_encoder(at.device);
    int ok = e->encode_windows(dev_base, n, byte_offsets, step, offsets, hip_stream);
    if (ok && out) {
        if (offsets[n] > cap) { pf::set_error("pf_deflate_tiles_device: the streams have " + std::to_string(offsets[n]) + " bytes, the buffer " + std::to_string(cap)); ok = 0; }
        else ok = e->fetch(out, hip_stream);
    }
    if (at.device != prev) (void)hipSetDevice(prev);
    return ok;
}
int pf_tiff_write_device_lossless(const char* filename, const void* dev_bgr, int rows, int cols, size_t step, const void* dev_mask, size_t mask_step, int bg,
                                  const double model_transform[16], int force_bigtiff, void* hip_stream)
{
    std::lock_guard<std::mutex> l(g_jpeg_mu);
    if (!filename || !dev_bgr || rows <= 0 || cols <= 0) { pf::set_error("pf_tiff_write_device_lossless: no name, no image or a size that is not positive"); return 0; }
    if (step == 0) step = (size_t)cols * 3;
    if (mask_step == 0) mask_step = (size_t)cols;
    if (step < (size_t)cols * 3 || (dev_mask && mask_step < (size_t)cols)) { pf::set_error("pf_tiff_write_device_lossless: step is smaller than a row"); return 0; }
    hipPointerAttribute_t at{}, am{};
    if (hipPointerGetAttributes(&at, dev_bgr) != hipSuccess || at.type != hipMemoryTypeDevice) { (void)hipGetLastError(); pf::set_error("pf_tiff_write_device_lossless: the image is not in device memory"); return 0; }
    if (dev_mask && (hipPointerGetAttributes(&am, dev_mask) != hipSuccess || am.type != hipMemoryTypeDevice || am.device != at.device)) {
        (void)hipGetLastError(); pf::set_error("pf_tiff_write_device_lossless: the mask is not in device memory beside the image"); return 0;
    }
    int prev = 0;
    (void)hipGetDevice(&prev);
    if (at.device != prev && hipSetDevice(at.device) != hipSuccess) { pf::set_error("pf_tiff_write_device_lossless: hipSetDevice failed"); return 0; }
    pf::TiffDevice::Mask mk;
    mk.dev_bytes = dev_mask; mk.step = mask_step;
    const int ok = shared_tiff_device(at.device)->write(filename, dev_bgr, rows, cols, step, 0, bg, model_transform, force_bigtiff != 0, *shared_jpeg_encoder(at.device), hip_stream,
                                                        dev_mask ? &mk : nullptr, shared_deflate_encoder(at.device));
    if (at.device != prev) (void)hipSetDevice(prev);
    return ok;
}
// pf_png_encode_device's encoder: one per device, as the JPEG one
static pf::PngEncoder* shared_png_encoder(int device)
{
    static pf::PngEncoder* e[64] = {};
    if (device < 0 || device >= 64) device = 0;
    if (!e[device]) e[device] = new pf::PngEncoder();
    return e[device];
}
int pf_png_encode_device(const void* dev_bgr, int rows, int cols, size_t step, const void* dev_mask, size_t mask_step, uint8_t* out, size_t cap, size_t* len, void* hip_stream)
{
    std::lock_guard<std::mutex> l(g_jpeg_mu);
    if (!len) { pf::set_error("pf_png_encode_device: no length"); return 0; }
    *len = 0;
    if (!pf::png_args_ok("pf_png_encode_device", dev_bgr, rows, cols, step, dev_mask, mask_step)) return 0;
    pf::png::Geometry g;
    (void)pf::png::geometry(rows, cols, dev_mask != nullptr, g);
    if (!out) { *len = (size_t)g.bound; return 1; }
    hipPointerAttribute_t at{}, am{};
    if (hipPointerGetAttributes(&at, dev_bgr) != hipSuccess || at.type != hipMemoryTypeDevice) { (void)hipGetLastError(); pf::set_error("pf_png_encode_device: the image is not in device memory"); return 0; }
    if (dev_mask && (hipPointerGetAttributes(&am, dev_mask) != hipSuccess || am.type != hipMemoryTypeDevice || am.device != at.device)) {
        (void)hipGetLastError(); pf::set_error("pf_png_encode_device: the mask is not in device memory beside the image"); return 0;
    }
    int prev = 0;
    (void)hipGetDevice(&prev);
    if (at.device != prev && hipSetDevice(at.device) != hipSuccess) { pf::set_error("pf_png_encode_device: hipSetDevice failed"); return 0; }
    pf::PngEncoder* e = shared_png_encoder(at.device);
    int ok = e->encode(dev_bgr, rows, cols, step, dev_mask, mask_step, len, hip_stream);
    if (ok) {
        if (*len > cap) { pf::set_error("pf_png_encode_device: the file has " + std::to_string(*len) + " bytes, the buffer " + std::to_string(cap)); ok = 0; }
        else ok = e->fetch(out, hip_stream);
    }
    if (at.device != prev) (void)hipSetDevice(prev);
    return ok;
}
void pf_debug_tiff_counts(pf_map* m, long long out[3])
{
    if (!out) return;
    size_t t = 0, e = 0, b = 0;
    if (m) m->impl.tiff_counts(&t, &e, &b);
    else {
        std::lock_guard<std::mutex> l(g_jpeg_mu);
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); dev = 0; }
        shared_tiff_device(dev)->last_counts(&t, &e, &b);
    }
    out[0] = (long long)t; out[1] = (long long)e; out[2] = (long long)b;
}
void pf_debug_jpeg_huffman(pf_map* m, long long out[3])
{
    if (!out) return;
    long a = 0, b = 0; int r = 0;
    if (m) m->jpeg.huffman_counts(&a, &b, &r);
    else { std::lock_guard<std::mutex> l(g_jpeg_mu); shared_jpeg()->huffman_counts(&a, &b, &r); }
    out[0] = a; out[1] = b; out[2] = r;
}
// one staged frame (JpegDevice slot i) into the map: the frame's slot in HBM is filled by the decoder's upload + kernels on the map's stream
static int feed_staged_jpeg(pf_map* m, int i, const double pose[7])
{
    int rows = 0, cols = 0;
    m->jpeg.staged_size(i, &rows, &cols);
    const FusionMap::FrameProducer fill = [m, i](void* dev, hipStream_t st) { return m->jpeg.submit(i, (uint8_t*)dev, (void*)st); };
    pf_image img = { rows, cols, PF_8UC3, nullptr, 0 };
    return m->impl.feed(&img, pose, false, &fill);
}
int pf_feed_jpeg(pf_map* m, const uint8_t* data, size_t len, const double pose[7])
{
    if (!m || !data || !pose) return 0;
    if (!m->impl.ok() || !m->impl.use_device()) { pf::set_error("pf_feed_jpeg: no device"); return 0; }
    unsigned char ok = 0;
    const int i = m->jpeg.stage_one(data, len, &ok);          // markers + Huffman on this thread, outside the map's lock
    if (!ok) { m->jpeg.submit(i, nullptr, nullptr); return 0; }          // leaves the frame's message in pf_last_error()
    return feed_staged_jpeg(m, i, pose);
}
int pf_feed_jpeg_batch(pf_map* m, int n, const uint8_t* const* data, const size_t* len, const double* poses7, int threads, int* results)
{
    if (!m || n < 1 || !data || !len || !poses7) return 0;
    int fed = 0;
    if (results) for (int i = 0; i < n; i++) results[i] = 0;
    if (!m->impl.ok() || !m->impl.use_device()) { pf::set_error("pf_feed_jpeg_batch: no device"); return 0; }
    for (int base = 0; base < n; base += pf::JpegDevice::kSlots) {
        const int cnt = std::min(n - base, (int)pf::JpegDevice::kSlots);
        unsigned char ok[pf::JpegDevice::kSlots];
        if (!m->jpeg.stage_batch(cnt, data + base, len + base, 0, 0, threads, ok)) return fed;
        for (int i = 0; i < cnt; i++) {
            if (!ok[i]) { m->jpeg.submit(i, nullptr, nullptr); continue; }
            const int r = feed_staged_jpeg(m, i, poses7 + 7 * (size_t)(base + i));
            if (results) results[base + i] = r;
            fed += r != 0;
        }
    }
    return fed;
}
int pf_save_to_memory(pf_map* m, uint8_t* bgr, int* rows, int* cols, int* tx0, int* ty0)
{ return m && rows && cols && tx0 && ty0 && m->impl.save_to_memory(bgr, rows, cols, tx0, ty0); }

int pf_save_to_memory_mask(pf_map* m, uint8_t* bgr, uint8_t* mask, int* rows, int* cols, int* tx0, int* ty0)
{ return m && rows && cols && tx0 && ty0 && m->impl.save_to_memory_mask(bgr, mask, rows, cols, tx0, ty0); }

int pf_num_levels(pf_map* m) { return m ? m->impl.num_levels() : 0; }
int pf_pyramid_type(pf_map* m) { return m ? m->impl.pyramid_type() : 0; }
int pf_grid(pf_map* m, int dims[4], double geo[6]) { return m && m->impl.grid(dims, geo); }
int pf_tile_count(pf_map* m) { return m ? m->impl.tile_count() : 0; }
int pf_tile_coords(pf_map* m, int* xy, int cap) { return m ? m->impl.tile_coords(xy, cap) : 0; }
int pf_get_tile_level(pf_map* m, int ix, int iy, int level, void* lap, float* w) { return m && m->impl.get_tile_level(ix, iy, level, lap, w); }
int pf_get_tile_bgra(pf_map* m, int ix, int iy, uint8_t* bgra) { return m && bgra && m->impl.get_tile_bgra(ix, iy, bgra); }
int pf_blend_tile_raw(pf_map* m, int ix, int iy, void* out) { return m && out && m->impl.blend_tile(ix, iy, out, nullptr, nullptr); }
int pf_blend_tile(pf_map* m, int ix, int iy, uint8_t* bgr) { return m && bgr && m->impl.blend_tile(ix, iy, nullptr, bgr, nullptr); }
int pf_blend_changed(pf_map* m, int* xy, uint8_t* bgr, int cap) { return (m && xy && bgr && cap > 0) ? m->impl.blend_changed(xy, bgr, cap) : 0; }
int pf_blend_tiles(pf_map* m, const int* xy, int n, uint8_t* bgr)
{
    if (!m || !xy || !bgr || n <= 0) return 0;
    std::vector<std::pair<int, int>> tiles(n);
    for (int i = 0; i < n; i++) tiles[i] = { xy[2 * i], xy[2 * i + 1] };
    return m->impl.blend_list(tiles, bgr);
}
int pf_blend_tiles_level(pf_map* m, const int* xy, int n, int level, uint8_t* bgr, void* raw)
{
    if (!m || !xy || (!bgr && !raw) || n <= 0) return 0;
    std::vector<std::pair<int, int>> tiles(n);
    for (int i = 0; i < n; i++) tiles[i] = { xy[2 * i], xy[2 * i + 1] };
    return m->impl.blend_list_level(tiles, level, bgr, raw);
}
int pf_blend_changed_level(pf_map* m, int level, int* xy, uint8_t* bgr, int cap) { return (m && xy && bgr && cap > 0) ? m->impl.blend_changed(xy, bgr, cap, level) : 0; }
int pf_save_to_memory_level(pf_map* m, int level, uint8_t* bgr, int* rows, int* cols, int* tx0, int* ty0)
{ return m && rows && cols && tx0 && ty0 && m->impl.save_to_memory_level(level, bgr, rows, cols, tx0, ty0); }
int pf_blend_tiles_jpeg(pf_map* m, const int* xy, int n, int quality, uint8_t* out, size_t cap, size_t* offsets)
{
    if (!m || !xy || !out || !offsets || n <= 0) { pf::set_error("pf_blend_tiles_jpeg: no map, no tiles or no buffer"); return 0; }
    std::vector<std::pair<int, int>> tiles(n);
    for (int i = 0; i < n; i++) tiles[i] = { xy[2 * i], xy[2 * i + 1] };
    return m->impl.blend_list_jpeg(tiles, quality, out, cap, offsets);
}
void* pf_host_alloc(size_t bytes)
{
    void* p = nullptr;
    // portable: page-locked for every device of the process (a node's maps live on different GPUs)
    if (!bytes || hipHostMalloc(&p, bytes, hipHostMallocPortable) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return p;
}
void pf_host_free(void* p) { if (p) (void)hipHostFree(p); }

// MultiBandMap2DCPUEle::normalizeUsingWeightMap / mulWeightMap (.cpp:57-75): no caller in
// the reference; host loops kept for API completeness.
int pf_normalize_using_weight_map(const float* weight, float* src3, size_t npix)
{
    if (!weight || !src3) return 0;
    for (size_t i = 0; i < npix; i++) {
        const float d = (float)(weight[i] + 1e-5);
        const float inv = 1.f / d;          // Point3_ operator/ multiplies by the reciprocal (Point.h:213-216)
        src3[3 * i] = inv * src3[3 * i]; src3[3 * i + 1] = inv * src3[3 * i + 1]; src3[3 * i + 2] = inv * src3[3 * i + 2];
    }
    return 1;
}
int pf_mul_weight_map(const float* weight, float* src3, size_t npix)
{
    if (!weight || !src3) return 0;
    for (size_t i = 0; i < npix; i++) { const float w = weight[i]; src3[3 * i] = w * src3[3 * i]; src3[3 * i + 1] = w * src3[3 * i + 1]; src3[3 * i + 2] = w * src3[3 * i + 2]; }
    return 1;
}

static pf::Pose to_pose(const double a[7]) { return pf::pose_from7(a); }
static void from_pose(const pf::Pose& p, double o[7]) { std::memcpy(o, p.t, 24); std::memcpy(o + 3, p.q, 32); }
// pi::calcLngLatFromDistance, PIL/src/hardware/Gps/utils_GPS.cpp:133-160 (same operations in the same order; DEG2RAD is the
// reference's truncated constant)
void pf_lnglat_from_distance(double lng1, double lat1, double dx, double dy, double* lng2, double* lat2)
{
    const double kEarthRadius = 6378137.0, kDeg2Rad = 0.017453292519943;
    const double a = kEarthRadius, f = 1.0 / 298.257223563, e_2 = 2 * f - f * f;
    const double phi_rad = lat1 * kDeg2Rad;
    const double sp = std::sin(phi_rad);
    const double lng_unit = kDeg2Rad * a * std::cos(phi_rad) / std::sqrt(1 - e_2 * (sp * sp));
    const double lat_unit = kDeg2Rad * a * (1 - e_2) / std::pow(1 - e_2 * (sp * sp), 1.5);
    if (lng2) *lng2 = dx / lng_unit + lng1;
    if (lat2) *lat2 = dy / lat_unit + lat1;
}

// MultiBandMap2DCPU.cpp:709-712 + :747-755
int pf_format_map_update(const double plane[7], const double gps_origin[3], double min_x, double min_y, double ele_size,
                         int x, int y, char* out, int cap)
{
    if (!plane || !gps_origin || !out || cap <= 0) return 0;
    const float x0 = (float)(min_x + x * ele_size), y0 = (float)(min_y + y * ele_size);
    const float x1 = (float)(x0 + ele_size), y1 = (float)(y0 + ele_size);
    const pf::Pose pl = to_pose(plane);
    double gps[2][2];
    const float cx[2] = { x0, x1 }, cy[2] = { y0, y1 };
    for (int k = 0; k < 2; k++) {
        const double p[3] = { (double)cx[k], (double)cy[k], 0.0 };
        double r[3];
        pf::rotate(pl.q, p, r);                                   // SE3 * Point3d = translation + rotation * p (SE3.h:99-101)
        pf_lnglat_from_distance(gps_origin[0], gps_origin[1], pl.t[0] + r[0], pl.t[1] + r[1], &gps[k][0], &gps[k][1]);
    }
    // std::to_string(double) is "%f"
    const int n = std::snprintf(out, (size_t)cap, "Map2DUpdate LastTexMat %f %f %f %f %f %f", gps[0][0], gps[0][1], 0.0, gps[1][0], gps[1][1], 0.0);
    return (n > 0 && n < cap) ? n : 0;
}

int pf_map_update_command(pf_map* m, int ix, int iy, const double gps_origin[3], char* out, int cap)
{
    if (!m || !gps_origin || !out) return 0;
    double plane[7], mn[2], ele; int x, y;
    if (!m->impl.map_update_inputs(ix, iy, plane, mn, &ele, &x, &y)) return 0;
    return pf_format_map_update(plane, gps_origin, mn[0], mn[1], ele, x, y, out, cap);
}

// --- Web-Mercator map tiles (webtiles_plan.hpp: the plan, pure host code; webtiles.hip: the kernels and the pyramid)
int pf_webtiles_georef_compose(const double model_transform[16], const double plane[7], const double gps_origin[3], double px2ll[6])
{
    if (!model_transform || !plane || !gps_origin || !px2ll) { pf::set_error("pf_webtiles_georef_compose: a null argument"); return 0; }
    double p[6], A[4];
    pf::webtiles::georef_compose(model_transform, plane, gps_origin, p);
    if (!pf::webtiles::invert2(p, A)) { pf::set_error(std::string("pf_webtiles_georef_compose: ") + pf::webtiles::plan_message(pf::webtiles::kPlanSingular)); return 0; }
    std::memcpy(px2ll, p, sizeof p);
    return 1;
}
int pf_webtiles_georef(pf_map* m, const double gps_origin[3], double px2ll[6], int* rows, int* cols)
{
    if (!m || !gps_origin || !px2ll) { pf::set_error("pf_webtiles_georef: no map, no origin or no result"); return 0; }
    return m->impl.webtiles_georef(gps_origin, px2ll, rows, cols);
}
int pf_webtiles_plan(const double px2ll[6], int rows, int cols, int z, int range[4], double* ux, double* uy, double* vx, double* vy, long long cap_cols, long long cap_rows)
{
    const pf::webtiles::PlanResult r = pf::webtiles::plan(px2ll, rows, cols, z, range, ux, uy, vx, vy, cap_cols, cap_rows);
    if (r != pf::webtiles::kPlanOk) { pf::set_error(std::string("pf_webtiles_plan: ") + pf::webtiles::plan_message(r)); return 0; }
    return 1;
}
int pf_webtiles_native_zoom(const double px2ll[6], int rows, int cols) { return pf::webtiles::native_zoom(px2ll, rows, cols); }
int pf_debug_webtiles_batch(int edge) { pf::webtiles_set_batch(edge); return pf::webtiles_batch(); }
void pf_debug_webtiles_timing(int on) { pf::webtiles_set_timing(on != 0); }
void pf_debug_webtiles_timing_read(double out4[4]) { if (out4) pf::webtiles_last_timing(out4); }
int pf_webtiles_device(const void* dev_bgr, int rows, int cols, size_t step, const void* dev_mask, size_t mask_step, const double px2ll[6], int zmin, int zmax, int quality, int bg,
                       int want_pixels, pf_webtile_sink sink, void* user, void* hip_stream)
{
    std::lock_guard<std::mutex> l(g_jpeg_mu);
    if (!dev_bgr || !dev_mask || !px2ll || !sink || rows <= 0 || cols <= 0) { pf::set_error("pf_webtiles_device: no image, no mask, no georeference, no sink or a size that is not positive"); return 0; }
    if ((step && step < (size_t)cols * 3) || (mask_step && mask_step < (size_t)cols)) { pf::set_error("pf_webtiles_device: step is smaller than a row"); return 0; }
    hipPointerAttribute_t at{}, am{};
    if (hipPointerGetAttributes(&at, dev_bgr) != hipSuccess || at.type != hipMemoryTypeDevice) { (void)hipGetLastError(); pf::set_error("pf_webtiles_device: the image is not in device memory"); return 0; }
    if (hipPointerGetAttributes(&am, dev_mask) != hipSuccess || am.type != hipMemoryTypeDevice || am.device != at.device) {
        (void)hipGetLastError(); pf::set_error("pf_webtiles_device: the mask is not in device memory beside the image"); return 0;
    }
    int prev = 0;
    (void)hipGetDevice(&prev);
    if (at.device != prev && hipSetDevice(at.device) != hipSuccess) { pf::set_error("pf_webtiles_device: hipSetDevice failed"); return 0; }
    const int ok = pf::webtiles_export(dev_bgr, rows, cols, step, dev_mask, mask_step, px2ll, zmin, zmax, quality, bg, want_pixels != 0, sink, user, *shared_jpeg_encoder(at.device), (hipStream_t)hip_stream);
    if (at.device != prev) (void)hipSetDevice(prev);
    return ok;
}
int pf_webtiles(pf_map* m, const double gps_origin[3], int zmin, int zmax, int quality, int want_pixels, pf_webtile_sink sink, void* user)
{
    if (!m || !gps_origin || !sink) { pf::set_error("pf_webtiles: no map, no origin or no sink"); return 0; }
    const FusionMap::WebTilesJob job{ gps_origin, zmin, zmax, quality, want_pixels != 0, sink, user, nullptr };
    return m->impl.webtiles(job);
}

// pf_save_webtiles: the sink that writes dir/z/x/y.jpg (+ .pbm) and counts for tiles.json
namespace {
struct WebDir {
    std::string dir, failed;
    struct Zoom { int x0 = 0, y0 = 0, x1 = 0, y1 = 0; long long tiles = 0, partial = 0; };
    std::map<int, Zoom> zooms;
    static bool make_dir(const std::string& d) { return ::mkdir(d.c_str(), 0777) == 0 || errno == EEXIST; }
    static bool write_file(const std::string& name, const char* head, const uint8_t* data, size_t len)
    {
        std::FILE* f = std::fopen(name.c_str(), "wb");
        if (!f) return false;
        bool ok = (!head || std::fputs(head, f) >= 0) && std::fwrite(data, 1, len, f) == len;
        ok = std::fclose(f) == 0 && ok;
        return ok;
    }
    static int sink(void* user, const pf_webtile* t)
    {
        WebDir& w = *(WebDir*)user;
        const std::string dz = w.dir + "/" + std::to_string(t->z), dx = dz + "/" + std::to_string(t->x), stem = dx + "/" + std::to_string(t->y);
        if (!make_dir(dz) || !make_dir(dx) || !write_file(stem + ".jpg", nullptr, t->jpeg, t->jpeg_len) ||
            (t->mask8192 && !write_file(stem + ".pbm", "P4\n256 256\n", t->mask8192, 8192))) { w.failed = stem; return 0; }
        Zoom& q = w.zooms[t->z];
        if (!q.tiles) { q.x0 = q.x1 = t->x; q.y0 = q.y1 = t->y; }
        q.x0 = std::min(q.x0, t->x); q.x1 = std::max(q.x1, t->x); q.y0 = std::min(q.y0, t->y); q.y1 = std::max(q.y1, t->y);
        q.tiles++; q.partial += t->cover == 1;
        return 1;
    }
};
}  // namespace

int pf_save_webtiles(pf_map* m, const char* dir, const double gps_origin[3], int zmin, int zmax, int quality)
{
    if (!m || !dir || !gps_origin) { pf::set_error("pf_save_webtiles: no map, no directory or no origin"); return 0; }
    WebDir w;
    w.dir = dir;
    if (!WebDir::make_dir(w.dir)) { pf::set_error("pf_save_webtiles: cannot create " + w.dir); return 0; }
    double rep[8] = {};
    const FusionMap::WebTilesJob job{ gps_origin, zmin, zmax, quality, false, &WebDir::sink, &w, rep };
    if (!m->impl.webtiles(job)) {
        if (!w.failed.empty()) pf::set_error("pf_save_webtiles: cannot write tile " + w.failed);
        return 0;
    }
    // the bounds: the box of the four image corners, in degrees
    double west = 0, east = 0, south = 0, north = 0;
    for (int k = 0; k < 4; k++) {
        const double c = (k & 1) ? rep[7] : 0.0, r = (k & 2) ? rep[6] : 0.0;
        const double lng = rep[0] + rep[1] * c + rep[2] * r, lat = rep[3] + rep[4] * c + rep[5] * r;
        if (!k) { west = east = lng; south = north = lat; }
        west = std::min(west, lng); east = std::max(east, lng); south = std::min(south, lat); north = std::max(north, lat);
    }
    const std::string name = w.dir + "/tiles.json";
    std::FILE* f = std::fopen(name.c_str(), "w");
    if (!f) { pf::set_error("pf_save_webtiles: cannot open " + name); return 0; }
    std::fprintf(f, "{\n  \"scheme\": \"xyz\", \"crs\": \"EPSG:3857\", \"format\": \"jpg\", \"tile_size\": 256, \"mask_format\": \"pbm\",\n");
    std::fprintf(f, "  \"bounds\": [%.10f, %.10f, %.10f, %.10f],\n", west, south, east, north);
    std::fprintf(f, "  \"minzoom\": %d, \"maxzoom\": %d,\n  \"zooms\": [", w.zooms.empty() ? 0 : w.zooms.begin()->first, w.zooms.empty() ? 0 : w.zooms.rbegin()->first);
    bool first = true;
    for (auto& kv : w.zooms) {
        std::fprintf(f, "%s\n    {\"z\": %d, \"x0\": %d, \"y0\": %d, \"x1\": %d, \"y1\": %d, \"tiles\": %lld, \"partial\": %lld}", first ? "" : ",", kv.first, kv.second.x0, kv.second.y0,
                     kv.second.x1, kv.second.y1, kv.second.tiles, kv.second.partial);
        first = false;
    }
    std::fprintf(f, "\n  ]\n}\n");
    if (std::fclose(f) != 0) { pf::set_error("pf_save_webtiles: cannot write " + name); return 0; }
    return 1;
}

// --- views (view_plan.hpp: the plan, pure host code; view.hip: the kernels; map_view.cpp: the engine)
int pf_view_plan(const double V[9], int width, int height, int level, const int dims[4], const double geo[6], int num_levels, const int extent[4], pf_view_info* out)
{
    const pf::view::PlanResult r = pf::view::plan(V, width, height, level, dims, geo, num_levels, extent, out);
    if (r != pf::view::kOk) { pf::set_error(std::string("pf_view_plan: ") + pf::view::plan_message(r)); return 0; }
    return 1;
}
int pf_render_view(pf_map* m, const double V[9], int width, int height, int level, int channels, uint8_t* out, size_t step, pf_view_info* info)
{
    if (!m || !V || !out) { pf::set_error("pf_render_view: no map, no matrix or no buffer"); return 0; }
    FusionMap::ViewTarget t;
    t.kind = FusionMap::ViewTarget::Host; t.out = out; t.step = step; t.channels = channels;
    return m->impl.render_view(V, width, height, level, t, info);
}
int pf_render_view_device(pf_map* m, const double V[9], int width, int height, int level, int channels, void* dev_out, size_t step, void* hip_stream, pf_view_info* info)
{
    if (!m || !V || !dev_out) { pf::set_error("pf_render_view_device: no map, no matrix or no buffer"); return 0; }
    FusionMap::ViewTarget t;
    t.kind = FusionMap::ViewTarget::Device; t.out = (uint8_t*)dev_out; t.step = step; t.channels = channels;
    t.stream = (hipStream_t)hip_stream; t.has_stream = hip_stream != nullptr;
    return m->impl.render_view(V, width, height, level, t, info);
}
int pf_render_view_jpeg(pf_map* m, const double V[9], int width, int height, int level, int quality, uint8_t* out, size_t cap, size_t* len, pf_view_info* info)
{
    if (!m || !V || !len) { pf::set_error("pf_render_view_jpeg: no map, no matrix or no length"); return 0; }
    if (!out) {
        if (width < 1 || width > pf::view::kMaxViewDim || height < 1 || height > pf::view::kMaxViewDim) { pf::set_error(std::string("pf_render_view_jpeg: ") + pf::view::plan_message(pf::view::kSize)); return 0; }
        *len = pf::jenc::stream_bound(height, width);
        return 1;
    }
    FusionMap::ViewTarget t;
    t.kind = FusionMap::ViewTarget::Jpeg; t.out = out; t.channels = 3; t.quality = quality; t.cap = cap; t.len = len;
    return m->impl.render_view(V, width, height, level, t, info);
}
int pf_view_of_extent(pf_map* m, int width, int height, double V[9]) { return m && V && m->impl.view_of_extent(width, height, V); }
int pf_view_from_pose(pf_map* m, const double pose_world7[7], const double* cam6_or_null, double V[9]) { return m && pose_world7 && V && m->impl.view_from_pose(pose_world7, cam6_or_null, V); }
int pf_view_from_lnglat(pf_map* m, const double gps_origin[3], double lng_w, double lat_n, double lng_e, double lat_s, int width, int height, double V[9])
{ return m && gps_origin && V && m->impl.view_from_lnglat(gps_origin, lng_w, lat_n, lng_e, lat_s, width, height, V); }
void pf_debug_view_timing(pf_map* m, int on) { if (m) m->impl.view_timing(on != 0); }
void pf_debug_view_timing_read(pf_map* m, double out4[4]) { if (m && out4) m->impl.view_timing_read(out4); }

void pf_se3_inverse(const double a[7], double out[7]) { from_pose(pf::inverse(to_pose(a)), out); }
void pf_se3_mul(const double a[7], const double b[7], double out[7]) { from_pose(pf::mul(to_pose(a), to_pose(b)), out); }
void pf_so3_rotate(const double q[4], const double p[3], double out[3]) { pf::rotate(q, p, out); }
int pf_footprint(const double cam[6], const double pose_plane[7], double pts8[8])
{
    const pf::Camera c{ cam[0], cam[1], cam[2], cam[3], cam[4], cam[5], 1. / cam[2], 1. / cam[3] };
    return pf::footprint(c, to_pose(pose_plane), pts8) ? 1 : 0;
}
void pf_perspective_transform(const float src8[8], const float dst8[8], double M[9]) { pf::perspective_transform(src8, dst8, M); }

int pf_tile_owner(const pf_options* o, int ix, int iy) { return o ? pf::tile_owner(o->shard_count, o->shard_block, ix, iy) : 0; }
size_t pf_halo_bytes(pf_map* m, int dx, int dy) { return m ? m->impl.halo_bytes_for(dx, dy) : 0; }
int pf_halo_pack(pf_map* m, int ix, int iy, int dx, int dy, void* dev_out) { return m && dev_out && m->impl.halo_pack(ix, iy, dx, dy, dev_out); }
int pf_blend_tile_halo(pf_map* m, int ix, int iy, const void* const dev_halo[9], uint8_t* bgr, void* raw)
{ return m && (bgr || raw) && m->impl.blend_tile(ix, iy, raw, bgr, dev_halo); }
size_t pf_tile_bytes(pf_map* m) { return m ? m->impl.tile_bytes() : 0; }
int pf_tile_export(pf_map* m, int ix, int iy, void* dev_out) { return m && dev_out && m->impl.tile_export(ix, iy, dev_out); }
int pf_tile_import(pf_map* m, int ix, int iy, const void* dev_in) { return m && dev_in && m->impl.tile_import(ix, iy, dev_in); }

// --- map merge, state file (map_merge.cpp, merge.hip, state_file.hpp)
int pf_merge(pf_map* dst, pf_map* src)
{
    if (!dst || !src) { pf::set_error("pf_merge: null map"); return 0; }
    return dst->impl.merge_from(src->impl);
}
int pf_merge_tiles(pf_map* m, int n, const int* xy, const void* const* dev_slots, const float* wlb16) { return m && m->impl.merge_tiles(n, xy, dev_slots, wlb16); }
int pf_tile_bounds(pf_map* m, int ix, int iy, float wlb16[16]) { return m && wlb16 && m->impl.tile_bounds(ix, iy, wlb16); }
int pf_save_state(pf_map* m, const char* path) { return m && path && m->impl.save_state(path); }
int pf_load_state(pf_map* m, const char* path) { return m && path && m->impl.load_state(path); }
int pf_merge_state(pf_map* m, const char* path) { return m && path && m->impl.merge_state(path); }
int pf_state_info(const char* path, int info[8], double plane[7], double cam[6], double geo[6])
{
    pf::statefile::StateHeader h; std::string why;
    if (!pf::statefile::scan_path(path, h, nullptr, why)) { pf::set_error("pf_state_info: " + why); return 0; }
    if (h.n_tiles > 0x7fffffffull) { pf::set_error("pf_state_info: more tiles than the count can say"); return 0; }
    if (info) { info[0] = h.map_type; info[1] = h.pyramid_type; info[2] = h.band_number; info[3] = h.weight_type; info[4] = (int)h.n_tiles; info[5] = h.w; info[6] = h.h; info[7] = (int)h.version; }
    if (plane) std::memcpy(plane, h.plane, sizeof(h.plane));
    if (cam) std::memcpy(cam, h.cam, sizeof(h.cam));
    if (geo) { geo[0] = h.min[0]; geo[1] = h.min[1]; geo[2] = h.max[0]; geo[3] = h.max[1]; geo[4] = h.ele_size; geo[5] = h.length_pixel; }
    return 1;
}
void pf_debug_merge_stats(pf_map* m, int count_stores, double out[6]) { if (m) m->impl.merge_stats(count_stores, out); }

// --- raw frames (raw_convert.hpp, raw_convert.hip)
// pf_raw_to_bgr: image_io.cpp (host code without a HIP dependency)
int pf_raw_to_bgr_device(const pf_raw_frame* src, void* dev_bgr, size_t bgr_step, void* hip_stream)
{
    std::string why;
    if (!src || !dev_bgr) { pf::set_error("pf_raw_to_bgr_device: no frame or no destination"); return 0; }
    if (!pf::raw::check(*src, why) || !pf::raw::check_bgr(*src, bgr_step, why)) { pf::set_error("pf_raw_to_bgr_device: " + why); return 0; }
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, dev_bgr) != hipSuccess || at.type != hipMemoryTypeDevice) { (void)hipGetLastError(); pf::set_error("pf_raw_to_bgr_device: destination is not device memory"); return 0; }
    const int device = at.device;
    for (int k = 0; k < pf::raw::planes_of(src->format); k++)
        if (hipPointerGetAttributes(&at, src->plane[k]) != hipSuccess || at.type != hipMemoryTypeDevice || at.device != device) {
            (void)hipGetLastError(); pf::set_error("pf_raw_to_bgr_device: plane " + std::to_string(k) + " is not memory of the destination's device"); return 0;
        }
    int prev = 0;
    (void)hipGetDevice(&prev);
    if (device != prev && hipSetDevice(device) != hipSuccess) { pf::set_error("pf_raw_to_bgr_device: hipSetDevice failed"); return 0; }
    pf::launch_raw_convert((hipStream_t)hip_stream, *src, (uint8_t*)dev_bgr, bgr_step);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) pf::set_error(std::string("pf_raw_to_bgr_device: ") + hipGetErrorString(e));
    if (device != prev) (void)hipSetDevice(prev);
    return e == hipSuccess;
}
int pf_feed_raw(pf_map* m, const pf_raw_frame* src, const double pose[7]) { return m && m->impl.feed_raw(src, pose, false); }
int pf_feed_raw_device(pf_map* m, const pf_raw_frame* src, const double pose[7]) { return m && m->impl.feed_raw(src, pose, true); }

// --- undistortion (undistort_plan.hpp, undistort.hip)
static bool undistort_cameras(const char* who, const double* in, int n, const double* out6, pf::undistort::InCamera& ic, pf::undistort::OutCamera& oc)
{
    if (!pf::undistort::make_camera(in, n, ic)) {
        pf::set_error(std::string(who) + ": the input camera needs 6 (PinHole), 7 (ATAN) or 11 (OpenCV) finite parameters, w, h >= 1, fx, fy != 0");
        return false;
    }
    if (!pf::undistort::make_out_camera(out6, oc)) { pf::set_error(std::string(who) + ": the output camera needs six finite numbers, w, h >= 1, fx, fy != 0"); return false; }
    return true;
}
int pf_undistort_table(const double* in, int n, const double out6[6], float* x, float* y, long long* uncovered)
{
    pf::undistort::InCamera ic; pf::undistort::OutCamera oc;
    if (!undistort_cameras("pf_undistort_table", in, n, out6, ic, oc)) return 0;
    const long long u = pf::undistort::build_table(ic, oc, x, y);
    if (uncovered) *uncovered = u;
    return 1;
}
int pf_undistort_fit_camera(const double* in, int n, double out6[6])
{
    pf::undistort::InCamera ic; pf::undistort::OutCamera oc;
    if (!undistort_cameras("pf_undistort_fit_camera", in, n, out6, ic, oc)) return 0;
    const int k = pf::undistort::fit_scale(ic, oc);
    if (!k) { pf::set_error("pf_undistort_fit_camera: no focal length up to 64 times the wanted one has the border covered"); return 0; }
    const pf::undistort::OutCamera f = pf::undistort::scaled(oc, k);
    out6[2] = f.fx; out6[3] = f.fy;
    return 1;
}
// the table of the most recent (in, out) pair of pf_undistort_bgr / _device, in the memory of the device it was used on
static std::mutex g_und_mu;
static struct { std::vector<double> key; int device = -1; void* table = nullptr; } g_und;
static const float2* undistort_device_table(const char* who, const double* in, int n, const double* out6, int device, pf::undistort::InCamera& ic, pf::undistort::OutCamera& oc)
{
    if (!undistort_cameras(who, in, n, out6, ic, oc)) return nullptr;
    std::vector<double> key(in, in + n);
    key.insert(key.end(), out6, out6 + 6);
    if (g_und.table && g_und.device == device && g_und.key == key) return (const float2*)g_und.table;
    const size_t pitch = pf::undistort_pitch(oc.w);
    std::vector<float2> tab(pitch * (size_t)oc.h, float2{ -1.f, -1.f });
    for (int y = 0; y < oc.h; y++)
        for (int x = 0; x < oc.w; x++) { float2& e = tab[(size_t)y * pitch + x]; (void)pf::undistort::entry(ic, oc, x, y, e.x, e.y); }
    if (g_und.table) { (void)hipFree(g_und.table); g_und.table = nullptr; }         // (waits for the kernels that read it)
    void* p = nullptr;
    if (hipMalloc(&p, tab.size() * sizeof(float2)) != hipSuccess || hipMemcpy(p, tab.data(), tab.size() * sizeof(float2), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        if (p) (void)hipFree(p);
        pf::set_error(std::string(who) + ": no device memory for the remap table");
        return nullptr;
    }
    g_und.key = key; g_und.device = device; g_und.table = p;
    return (const float2*)p;
}
static bool undistort_source_ok(const char* who, const pf::undistort::InCamera& ic, const pf_image* src, int out_w, size_t& src_step, size_t& dst_step)
{
    if (!src || !src->data || (src->type != PF_8UC3 && src->type != PF_8UC4) || src->cols != ic.w || src->rows != ic.h) {
        pf::set_error(std::string(who) + ": the source is not a BGR8 / BGRA8 frame of the input camera's size"); return false;
    }
    const size_t row = (size_t)src->cols * (src->type == PF_8UC4 ? 4 : 3);
    src_step = src->step ? src->step : row;
    if (dst_step == 0) dst_step = (size_t)out_w * 3;
    if (src_step < row || dst_step < (size_t)out_w * 3) { pf::set_error(std::string(who) + ": a row step is smaller than a row"); return false; }
    return true;
}
int pf_undistort_device(const double* in, int n, const double out6[6], const pf_image* src, void* dst, size_t dst_step, void* hip_stream)
{
    std::lock_guard<std::mutex> l(g_und_mu);
    if (!dst) { pf::set_error("pf_undistort_device: no destination"); return 0; }
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, dst) != hipSuccess || at.type != hipMemoryTypeDevice) { (void)hipGetLastError(); pf::set_error("pf_undistort_device: destination is not device memory"); return 0; }
    int prev = 0;
    (void)hipGetDevice(&prev);
    if (at.device != prev && hipSetDevice(at.device) != hipSuccess) { pf::set_error("pf_undistort_device: hipSetDevice failed"); return 0; }
    pf::undistort::InCamera ic; pf::undistort::OutCamera oc;
    size_t src_step = 0;
    int ok = 0;
    const float2* table = undistort_device_table("pf_undistort_device", in, n, out6, at.device, ic, oc);
    if (table && undistort_source_ok("pf_undistort_device", ic, src, oc.w, src_step, dst_step)) {
        pf::launch_undistort((hipStream_t)hip_stream, (const uint8_t*)src->data, src_step, ic.w, ic.h, src->type == PF_8UC4 ? 4 : 3, table, (uint8_t*)dst, dst_step, oc.w, oc.h);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) pf::set_error(std::string("pf_undistort_device: ") + hipGetErrorString(e));
        ok = e == hipSuccess;
    }
    if (at.device != prev) (void)hipSetDevice(prev);
    return ok;
}
int pf_undistort_bgr(const double* in, int n, const double out6[6], const pf_image* src, uint8_t* dst, size_t dst_step)
{
    std::lock_guard<std::mutex> l(g_und_mu);
    if (!dst) { pf::set_error("pf_undistort_bgr: no destination"); return 0; }
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess) { (void)hipGetLastError(); pf::set_error("pf_undistort_bgr: no HIP device"); return 0; }
    pf::undistort::InCamera ic; pf::undistort::OutCamera oc;
    size_t src_step = 0;
    const float2* table = undistort_device_table("pf_undistort_bgr", in, n, out6, device, ic, oc);
    if (!table || !undistort_source_ok("pf_undistort_bgr", ic, src, oc.w, src_step, dst_step)) return 0;
    const int cn = src->type == PF_8UC4 ? 4 : 3;
    const size_t src_bytes = (size_t)(ic.h - 1) * src_step + (size_t)ic.w * cn, out_row = (size_t)oc.w * 3;
    uint8_t *dsrc = nullptr, *ddst = nullptr;
    int ok = hipMalloc((void**)&dsrc, src_bytes) == hipSuccess && hipMalloc((void**)&ddst, out_row * oc.h) == hipSuccess &&
             hipMemcpy(dsrc, src->data, src_bytes, hipMemcpyHostToDevice) == hipSuccess;
    if (ok) {
        pf::launch_undistort(nullptr, dsrc, src_step, ic.w, ic.h, cn, table, ddst, out_row, oc.w, oc.h);
        ok = hipGetLastError() == hipSuccess && hipMemcpy2D(dst, dst_step, ddst, out_row, out_row, (size_t)oc.h, hipMemcpyDeviceToHost) == hipSuccess;
    }
    if (!ok) { pf::set_error(std::string("pf_undistort_bgr: ") + hipGetErrorString(hipGetLastError())); }
    if (dsrc) (void)hipFree(dsrc);
    if (ddst) (void)hipFree(ddst);
    return ok;
}
int pf_set_input_camera(pf_map* m, const double* in, int n) { return m && (n == 0 || in) && m->impl.set_input_camera(in, n); }
int pf_input_camera_info(pf_map* m, int* rows_in, int* cols_in, long long* uncovered) { return m && m->impl.input_camera_info(rows_in, cols_in, uncovered); }

// --- seam exchange (dist.cpp)
struct pf_dist { pf::DistMap impl; pf_map* owner; pf_dist(pf_map* m, pf::Transport* t) : impl(&m->impl, t), owner(m) {} };
int pf_dist_unique_id(void* out128) { return out128 && pf::rccl_unique_id(out128); }
pf_dist* pf_dist_init_rccl(pf_map* m, const void* id128, int rank, int nranks)
{
    if (!m || !id128 || nranks < 1 || rank < 0 || rank >= nranks) return nullptr;
    pf::Transport* t = pf::make_rccl_transport(id128, rank, nranks, m->impl.device());
    return t ? new (std::nothrow) pf_dist(m, t) : nullptr;
}
pf_dist* pf_dist_init_host(pf_map* m, int rank, int nranks, pf_exchange_fn fn, void* user)
{
    if (!m || !fn || nranks < 1 || rank < 0 || rank >= nranks) return nullptr;
    pf::Transport* t = pf::make_host_transport(rank, nranks, fn, user);
    return t ? new (std::nothrow) pf_dist(m, t) : nullptr;
}
void pf_dist_destroy(pf_dist* d) { delete d; }
int pf_dist_blend_changed(pf_dist* d, int* xy, uint8_t* bgr, int cap) { return (d && xy && bgr && cap >= 0) ? d->impl.blend_changed(xy, bgr, cap) : -1; }
// frame distribution moves frames of the map's own camera between the ranks: a map with an input camera is refused, nothing touched
static bool dist_refuses_input_camera(pf_dist* d, const char* who)
{
    if (!d->owner->impl.has_input_camera()) return false;
    pf::set_error(std::string(who) + ": the map has an input camera (pf_set_input_camera); undistort the frames first, or clear it");
    return true;
}
int pf_dist_feed(pf_dist* d, const pf_image* img, const double pose[7], int root)
{
    if (!d || !img || !pose || dist_refuses_input_camera(d, "pf_dist_feed")) return -1;
    return d->impl.feed(img, pose, root);
}
int pf_dist_feed_jpeg(pf_dist* d, const uint8_t* data, size_t len, int rows, int cols, const double pose[7], int root)
{
    if (!d || !pose || dist_refuses_input_camera(d, "pf_dist_feed_jpeg")) return -1;
    pf_image img = { rows, cols, PF_8UC3, nullptr, 0 };
    if (d->impl.rank() != root) return d->impl.feed(&img, pose, root);
    // the root: markers + (where the stream needs it) Huffman here, the rest queued on the map's stream into the staged slot
    pf_map* m = d->owner;
    unsigned char ok = 0; int i = -1;
    if (data && m->impl.ok() && m->impl.use_device()) i = m->jpeg.stage_one(data, len, &ok);
    const FusionMap::FrameProducer fill = [m, i, ok, rows, cols](void* dev, hipStream_t st) {
        int r = 0, c = 0;
        if (i < 0 || !ok) { if (i >= 0) m->jpeg.submit(i, nullptr, nullptr); else pf::set_error("pf_dist_feed_jpeg: the root has no stream"); return false; }
        m->jpeg.staged_size(i, &r, &c);
        if (r != rows || c != cols) { pf::set_error("pf_dist_feed_jpeg: the stream does not have the size announced to the ranks"); return false; }
        return m->jpeg.submit(i, (uint8_t*)dev, (void*)st);
    };
    return d->impl.feed(&img, pose, root, &fill);
}
int pf_dist_save_tiff_lossless(pf_dist* d, const char* filename, int masked, int force_bigtiff) { return d && filename && d->impl.save_tiff_lossless(filename, masked != 0, force_bigtiff != 0); }
int pf_dist_save(pf_dist* d, const char* filename) { return d && filename && d->impl.save(filename); }
int pf_dist_save_to_memory(pf_dist* d, uint8_t* bgr, int* rows, int* cols, int* tx0, int* ty0)
{ return d && rows && cols && tx0 && ty0 && d->impl.save_to_memory(bgr, rows, cols, tx0, ty0); }
int pf_dist_last_stats(pf_dist* d, pf_dist_stats* out) { if (!d || !out) return 0; *out = d->impl.stats(); return 1; }
int pf_dist_plan_blend(int nranks, int me, const int* counts, const int* lists3, const long long* caps, int high_quality,
                       const size_t halo_bytes9[9], pf_strip_plan* send, int send_cap, int* n_send,
                       pf_strip_plan* recv, int recv_cap, int* n_recv, int* mine_xy, int mine_cap, int* n_mine)
{
    if (nranks < 1 || me < 0 || me >= nranks || !counts || !lists3 || !caps || !halo_bytes9 || !n_send || !n_recv || !n_mine) return 0;
    std::vector<std::vector<pf::FusionMap::TileRec>> all(nranks);
    std::vector<long long> cp(caps, caps + nranks);
    const int* q = lists3;
    for (int r = 0; r < nranks; r++)
        for (int k = 0; k < counts[r]; k++, q += 3) all[r].push_back({ q[0], q[1], q[2] });
    pf::BlendPlan plan;
    pf::plan_blend(all, cp, me, high_quality != 0, halo_bytes9, plan);
    int ns = 0, nr = (int)plan.wants.size(), nm = (int)plan.mine.size();
    for (auto& v : plan.send_req) ns += (int)v.size();
    *n_send = ns; *n_recv = nr; *n_mine = nm;
    if (ns > send_cap || nr > recv_cap || nm > mine_cap || (ns && !send) || (nr && !recv) || (nm && !mine_xy)) return 0;
    int i = 0;
    for (int p = 0; p < nranks; p++)
        for (auto& rq : plan.send_req[p]) send[i++] = pf_strip_plan{ p, rq.ix, rq.iy, rq.dx, rq.dy, -1, (unsigned long long)rq.out_off };
    for (int k = 0; k < nr; k++) {
        const auto& w = plan.wants[k];
        recv[k] = pf_strip_plan{ w.peer, plan.mine[w.tile].first, plan.mine[w.tile].second, w.j % 3 - 1, w.j / 3 - 1, w.tile, (unsigned long long)w.off };
    }
    for (int k = 0; k < nm; k++) { mine_xy[2 * k] = plan.mine[k].first; mine_xy[2 * k + 1] = plan.mine[k].second; }
    return 1;
}
int pf_dist_set_verify(pf_dist* d, int on) { if (!d) return 0; d->impl.set_verify(on != 0); return 1; }
int pf_dist_info(pf_dist* d, int* rank, int* nranks, const char** transport)
{
    if (!d) return 0;
    const pf::Transport* t = d->impl.transport();
    if (rank) *rank = t->rank;
    if (nranks) *nranks = t->nranks;
    if (transport) *transport = t->name();
    return 1;
}

int pf_profile_enable(pf_map* m, int mode) { if (!m) return 0; m->impl.profile_enable(mode); return 1; }
int pf_profile_read(pf_map* m, int cap, const char** names, double* total_ms, long long* launches, double* alg_bytes)
{ return m ? m->impl.profile_read(cap, names, total_ms, launches, alg_bytes) : 0; }
int pf_profile_read_run(pf_map* m, int cap, const char** names, double* total_ms, long long* launches, double* alg_bytes, double* alg_bytes_run)
{ return m ? m->impl.profile_read(cap, names, total_ms, launches, alg_bytes, alg_bytes_run) : 0; }
int pf_profile_reset(pf_map* m) { if (!m) return 0; m->impl.profile_reset(); return 1; }
int pf_reserve_tiles(pf_map* m, long long n_tiles) { return m && m->impl.reserve_tiles(n_tiles) ? 1 : 0; }
int pf_render_stats(pf_map* m, double out4[4]) { if (!m || !out4) return 0; m->impl.render_stats(out4); return 1; }
int pf_stats(pf_map* m, long long* rendered, long long* rejected, long long* dropped) { if (!m) return 0; m->impl.stats(rendered, rejected, dropped); return 1; }
int pf_stats_failed(pf_map* m, long long* rendered, long long* rejected, long long* dropped, long long* failed)
{ if (!m) return 0; m->impl.stats(rendered, rejected, dropped, failed); return 1; }
int pf_timer_read(pf_map* m, int cap, const char** names, long long* calls, double* mean_s, double* min_s, double* max_s)
{
    return m ? m->impl.timer_read(cap, names, calls, mean_s, min_s, max_s) : 0;
}
int pf_timer_reset(pf_map* m) { if (!m) return 0; m->impl.timer_reset(); return 1; }

}  // extern "C"
