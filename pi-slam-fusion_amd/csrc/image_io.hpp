// image_io.hpp -- what image_io.cpp (host only) offers the engine: the route of a save and the host writers
#pragma once
#include <cstddef>
#include <cstdint>

namespace pf {

// Who turns the collapsed mosaic into the file save() was asked for: the GPU encoders, which read it where it lies in HBM
// (multi-band maps), or a host writer, which takes it as pixels.
enum class SaveRoute {
    DeviceJpeg,      // jpeg_encode.hip: only the stream comes to the host
    DeviceTiff,      // overview.hip + jpeg_encode.hip: the tiled pyramid TIFF
    HostTiffGeo,     // write_tiff_file with the map's quality, background and ModelTransformationTag (single-band maps)
    HostImage,       // write_image_file: PNG, PPM, and a single-band map's JPEG
    DeviceTiffLossless,   // overview.hip + deflate_encode.hip: the pyramid TIFF with Deflate tiles (pf_save_tiff_lossless; no file name asks for it)
    HostTiffLossless,     // write_tiff_lossless_file with the map's background, transform and alpha coverage (single-band maps)
    DevicePng,            // png_encode.hip: the PNG of pf_save_png, complete in HBM (no file name asks for it)
    HostPng,              // write_png_file: the same file by the scalar encoder, alpha from the tiles' alpha bytes (single-band maps)
};
// THE decision, from the name's extension (either case) and the map's kind; pf_save_tiff's "a TIFF under any name" is tiff_route
SaveRoute save_route(const char* filename, bool single_band);
inline SaveRoute tiff_route(bool single_band) { return single_band ? SaveRoute::HostTiffGeo : SaveRoute::DeviceTiff; }
inline SaveRoute tiff_lossless_route(bool single_band) { return single_band ? SaveRoute::HostTiffLossless : SaveRoute::DeviceTiffLossless; }
inline SaveRoute png_route(bool single_band) { return single_band ? SaveRoute::HostPng : SaveRoute::DevicePng; }
inline bool route_on_device(SaveRoute r) { return r == SaveRoute::DeviceJpeg || r == SaveRoute::DeviceTiff || r == SaveRoute::DeviceTiffLossless || r == SaveRoute::DevicePng; }

// PNG (zlib) / PPM / JPEG / plain TIFF by the name, as cv::imwrite picks
bool write_image_file(const char* filename, const uint8_t* bgr, int rows, int cols);
bool write_tiff_file(const char* who, const char* filename, const uint8_t* bgr, int rows, int cols, size_t step, int quality, int bg, const double* model_transform, bool force_bigtiff);
// the masked file (pf_tiff_write_bgr_masked): mask is a byte per pixel, non-zero = covered, rows of mask_step bytes (0 = packed)
bool write_tiff_masked_file(const char* who, const char* filename, const uint8_t* bgr, int rows, int cols, size_t step, const uint8_t* mask, size_t mask_step,
                            int quality, int bg, const double* model_transform, bool force_bigtiff);
// the lossless file (pf_tiff_write_bgr_lossless): Deflate tiles; mask may be null (the unmasked file)
bool write_tiff_lossless_file(const char* who, const char* filename, const uint8_t* bgr, int rows, int cols, size_t step, const uint8_t* mask, size_t mask_step,
                              int bg, const double* model_transform, bool force_bigtiff);
// the PNG of pf_png_encode_bgr (png_encode.hpp) as a file; mask may be null (an RGB file).  No file is left behind on failure
bool write_png_file(const char* who, const char* filename, const uint8_t* bgr, int rows, int cols, size_t step, const uint8_t* mask, size_t mask_step);
// what both PNG encoders refuse, said in `who`'s name; step and mask_step come back with 0 (packed) resolved
bool png_args_ok(const char* who, const void* bgr, int rows, int cols, size_t& step, const void* mask, size_t& mask_step);
bool jpeg_size_ok(const char* who, int rows, int cols);
bool write_bytes_file(const char* filename, const uint8_t* data, size_t len);

}  // namespace pf
