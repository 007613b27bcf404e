// Map2D.h -- C++ face of libpifusion.so with the reference's own interface
// (Map2DFusion/Map2D.h:37-98): PinHoleParameters, Map2D::create / prepare / feed /
// draw / save / queueSize, plus the MultiBandMap2DCPU::Ele tile surface
// (Map2DFusion/MultiBandMap2DCPU.h:32-51).  Header-only over the C ABI (pifusion.h),
// so there is exactly one binary boundary.
//
// Drop-in notes
//   * poses are taken from ANY type with get_translation() / get_rotation() whose
//     members are x,y,z(,w) -- the reference's own pi::SE3d works unchanged; a minimal
//     pi::SE3d is provided when GSLAM is not on the include path.
//   * images are taken from ANY type with rows, cols, type(), data (cv::Mat) or
//     rows, cols, type(), data (GSLAM::GImage); pixels are copied before feed() returns,
//     so the caller's refcounted buffer may go away (the reference keeps a cv::Mat
//     reference instead, MultiBandMap2DCPU.cpp:297-301).
//   * draw() has no GL here: it refreshes the blended tiles (the texture upload's
//     pixel work, .cpp:705-742) and hands them to an optional callback.
#ifndef PIFUSION_MAP2D_H
#define PIFUSION_MAP2D_H
#include "../pifusion.h"
#include <deque>
#include <functional>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#ifndef ELE_PIXELS
#define ELE_PIXELS 256
#endif

#ifndef GSLAM_SE3_H          // the reference's header defines pi::SE3d itself
namespace pi {
struct Point3d { double x = 0, y = 0, z = 0; Point3d() {} Point3d(double X, double Y, double Z) : x(X), y(Y), z(Z) {} };
struct SO3d { double x = 0, y = 0, z = 0, w = 1; SO3d() {} SO3d(double X, double Y, double Z, double W) : x(X), y(Y), z(Z), w(W) {} };
class SE3d {
public:
    SE3d() {}
    SE3d(double x, double y, double z, double wx, double wy, double wz, double w) : r_(wx, wy, wz, w), t_(x, y, z) {}
    SE3d(const SO3d& r, const Point3d& t) : r_(r), t_(t) {}
    const SO3d& get_rotation() const { return r_; }
    const Point3d& get_translation() const { return t_; }
private:
    SO3d r_; Point3d t_;
};
}  // namespace pi
#endif

struct PinHoleParameters {        // Map2DFusion/Map2D.h:37-43
    PinHoleParameters() {}
    PinHoleParameters(int _w, int _h, double _fx, double _fy, double _cx, double _cy)
        : w(_w), h(_h), fx(_fx), fy(_fy), cx(_cx), cy(_cy) {}
    double w = 0, h = 0, fx = 0, fy = 0, cx = 0, cy = 0;
};

namespace pifusion {

// non-owning image view with cv::Mat / GImage field names
struct ImageView {
    int rows = 0, cols = 0, flags = 0;
    unsigned char* data = nullptr;
    size_t step = 0;
    ImageView() {}
    ImageView(int r, int c, int t, void* d, size_t s = 0) : rows(r), cols(c), flags(t), data((unsigned char*)d), step(s) {}
    int type() const { return flags; }
};

template <class SE3> inline void pose7(const SE3& p, double o[7])
{
    const auto& t = p.get_translation(); const auto& r = p.get_rotation();
    o[0] = t.x; o[1] = t.y; o[2] = t.z; o[3] = r.x; o[4] = r.y; o[5] = r.z; o[6] = r.w;
}
// row pitch of the caller's image: cv::Mat::step (MatStep converts to size_t) and ImageView::step are carried over,
// so a ROI of a wider buffer or a row-padded image is read with its own pitch; types without a step member
// (GSLAM::GImage is always packed, GImage.h:387-389) give 0 = packed
template <class Img> inline auto step_of(const Img& m, int) -> decltype(size_t(m.step)) { return size_t(m.step); }
template <class Img> inline size_t step_of(const Img&, long) { return 0; }
template <class Img> inline pf_image view(const Img& m)
{
    pf_image v; v.rows = m.rows; v.cols = m.cols; v.type = m.type() & 0xfff; v.data = m.data; v.step = step_of(m, 0);
    return v;
}

}  // namespace pifusion

class Map2D {
public:
    enum Map2DType { NoType = 0, TypeCPU = 1, TypeGPU = 2, TypeMultiBandCPU = 3, TypeRender = 4 };   // Map2D.h:83

    // MultiBandMap2DCPU::MultiBandMap2DCPUEle, read side
    struct Ele {
        int ix = 0, iy = 0;
        std::vector<std::vector<unsigned char>> pyr_laplace;   // level i: (256>>i)^2 x 3 x {int16|float}
        std::vector<std::vector<float>> weights;               // level i: (256>>i)^2
    };

    static std::shared_ptr<Map2D> create(int type = TypeCPU, bool thread = true, const pf_options* opt = nullptr)
    {
        pf_map* h = pf_create(type, thread ? 1 : 0, opt);
        return h ? std::shared_ptr<Map2D>(new Map2D(h)) : std::shared_ptr<Map2D>();
    }
    ~Map2D() { pf_host_free(tex_); pf_destroy(h_); }
    Map2D(const Map2D&) = delete;
    Map2D& operator=(const Map2D&) = delete;

    template <class Img, class SE3>
    bool prepare(const SE3& plane, const PinHoleParameters& camera, const std::deque<std::pair<Img, SE3>>& frames)
    {
        double pl[7]; pifusion::pose7(plane, pl);
        const double cam[6] = { camera.w, camera.h, camera.fx, camera.fy, camera.cx, camera.cy };
        std::vector<double> poses(frames.size() * 7);
        std::vector<pf_image> imgs(frames.size());
        size_t i = 0;
        for (const auto& f : frames) { imgs[i] = pifusion::view(f.first); pifusion::pose7(f.second, &poses[7 * i]); i++; }
        return pf_prepare(h_, pl, cam, (int)frames.size(), imgs.data(), poses.data()) != 0;
    }
    template <class Img, class SE3> bool feed(const Img& img, const SE3& pose)      // Map2D.h:91
    {
        double p[7]; pifusion::pose7(pose, p);
        const pf_image v = pifusion::view(img);
        return pf_feed(h_, &v, p) != 0;
    }
    // feed(cv::imread(file), pose) with the file's bytes instead of its pixels (backup/map2dfusion.cpp:129-135): the JPEG stream is
    // decoded straight into HBM (Huffman on this thread, IDCT / upsampling / colour on the GPU) and rendered from there
    template <class SE3> bool feedJpeg(const unsigned char* data, size_t len, const SE3& pose)
    {
        double p[7]; pifusion::pose7(pose, p);
        return pf_feed_jpeg(h_, data, len, p) != 0;
    }
    // feed() of the BGR picture a raw frame converts to -- NV12 / NV21 / I420, grey or Bayer, host planes (pf_feed_raw): the planes cross to
    // HBM as they are, 1 or 1.5 bytes a pixel, and are converted there; they may be released when the call returns
    template <class SE3> bool feedRaw(const pf_raw_frame& raw, const SE3& pose)
    {
        double p[7]; pifusion::pose7(pose, p);
        return pf_feed_raw(h_, &raw, p) != 0;
    }
    // The frames fed from now on are those of a distorted camera -- GSLAM parameters as Camera(std::vector<double>) reads them: 6 PinHole,
    // 7 ATAN, 11 OpenCV, with their own width and height -- and are undistorted on the GPU into the camera of prepare() before the map
    // sees them (the reference's dataset adapters call GSLAM::Undistorter for this).  An empty vector clears it.  Survives prepare(),
    // not loadState().  false: pf_last_error() says why, nothing changed
    bool setInputCamera(const std::vector<double>& paras) { return pf_set_input_camera(h_, paras.empty() ? nullptr : paras.data(), (int)paras.size()) != 0; }
    // draw(): refresh every tile whose Ischanged flag is set and pass (ix, iy, BGR8 256x256) on.
    // With fuseGoogle() set, `announce` receives what the reference hands to scommand.Call("MapWidget", ...) for every refreshed
    // tile that is not on the rim of the grid (MultiBandMap2DCPU.cpp:744-757): "Map2DUpdate LastTexMat <gpsTL> <gpsBR>".
    void draw(const std::function<void(int, int, const unsigned char*)>& sink = nullptr,
              const std::function<void(const std::string&)>& announce = nullptr)
    { drawLevel(0, sink, announce); }
    // draw() for a viewer that is zoomed out: the same tiles as views of pyramid level `level` (pf_blend_changed_level), BGR8
    // E x E with E = ELE_PIXELS >> level -- the GPU minifies, and 4^-level of the pixels cross to the host
    void drawLevel(int level, const std::function<void(int, int, const unsigned char*)>& sink = nullptr,
                   const std::function<void(const std::string&)>& announce = nullptr)
    {
        const int cap = pf_tile_count(h_);
        if (cap <= 0 || level < 0 || level > 8) return;
        std::vector<int> xy(2 * (size_t)cap);
        // the tiles come back in ONE launch and one PCIe transfer into a page-locked buffer that this object keeps between draws
        // (pf_host_alloc: filled straight from HBM; the textures updateTexture hands to GL, .cpp:159-176)
        const size_t tile = (size_t)(ELE_PIXELS >> level) * (ELE_PIXELS >> level) * 3;
        const size_t need = (size_t)cap * tile;
        if (tex_cap_ < need) {
            pf_host_free(tex_); tex_cap_ = 0;
            tex_ = (unsigned char*)pf_host_alloc(need + need / 4);
            if (!tex_) return;
            tex_cap_ = need + need / 4;
        }
        unsigned char* px = tex_;
        const int n = level ? pf_blend_changed_level(h_, level, xy.data(), px, cap) : pf_blend_changed(h_, xy.data(), px, cap);
        for (int i = 0; i < n; i++) {
            if (sink) sink(xy[2 * i], xy[2 * i + 1], px + (size_t)i * tile);
            char cmd[256];
            if (fuse2google_ && announce && pf_map_update_command(h_, xy[2 * i], xy[2 * i + 1], gps_origin_, cmd, (int)sizeof cmd) > 0) announce(cmd);
        }
    }
    // svar "Fuse2Google" and "GPS.Origin" (longitude latitude altitude) of the reference (.cpp:196, :744)
    void fuseGoogle(bool on, double lng = 0, double lat = 0, double alt = 0) { fuse2google_ = on; gps_origin_[0] = lng; gps_origin_[1] = lat; gps_origin_[2] = alt; }
    // .png, .jpg / .jpeg, .tif / .tiff (tiled pyramid TIFF with JPEG tiles, overviews and geo tags), else PPM: see pf_save
    bool save(const std::string& filename) { return pf_save(h_, filename.c_str()) != 0; }
    // the mosaic as a tiled pyramid TIFF with lossless (Deflate, Predictor 2) tiles, under any name (pf_save_tiff_lossless)
    bool saveLossless(const std::string& filename, bool masked = false, bool force_bigtiff = false) { return pf_save_tiff_lossless(h_, filename.c_str(), masked, force_bigtiff) != 0; }
    // the mosaic as a PNG encoded on the GPU, under any name; masked: RGBA, transparent where save() paints the background (pf_save_png)
    bool savePng(const std::string& filename, bool masked = false) { return pf_save_png(h_, filename.c_str(), masked ? 1 : 0) != 0; }
    bool saveTiff(const std::string& filename, int quality = 95, bool force_bigtiff = false) { return pf_save_tiff(h_, filename.c_str(), quality, force_bigtiff ? 1 : 0) != 0; }
    // the pyramid TIFF with a transparency mask behind every image: covered where the level-0 weight is not 0 (pf_save_tiff_masked)
    bool saveMasked(const std::string& filename, int quality = 95, bool force_bigtiff = false) { return pf_save_tiff_masked(h_, filename.c_str(), quality, force_bigtiff ? 1 : 0) != 0; }
    // other's tiles merged into this map's on the GPU: this map ends as the map fed its own keyframes and then other's (pf_merge)
    bool merge(Map2D& other) { return pf_merge(h_, other.h_) != 0; }
    // the map's whole state in one file, "prepare from the file", and a file merged like a map (pf_save_state / pf_load_state / pf_merge_state)
    bool saveState(const std::string& filename) { return pf_save_state(h_, filename.c_str()) != 0; }
    bool loadState(const std::string& filename) { return pf_load_state(h_, filename.c_str()) != 0; }
    bool mergeState(const std::string& filename) { return pf_merge_state(h_, filename.c_str()) != 0; }
    // north-up Web-Mercator map tiles dir/z/x/y.jpg (+ .pbm coverage of partly covered tiles, tiles.json) around GPS.Origin (pf_save_webtiles);
    // zmax < 0: the native zoom, zmin < 0: down to the zoom at which one tile holds the mosaic
    bool saveWebTiles(const std::string& dir, const double gpsOrigin[3], int zmin = -1, int zmax = -1, int quality = 95)
    { return pf_save_webtiles(h_, dir.c_str(), gpsOrigin, zmin, zmax, quality) != 0; }
    unsigned queueSize() { return pf_queue_size(h_); }
    bool sync() { return pf_sync(h_) != 0; }

    // Ele access (D2H copy of one tile's pyramids)
    bool ele(int ix, int iy, Ele& e)
    {
        const int nl = pf_num_levels(h_), es = pf_pyramid_type(h_) == PF_32FC3 ? 4 : 2;
        e.ix = ix; e.iy = iy; e.pyr_laplace.resize(nl); e.weights.resize(nl);
        for (int i = 0; i < nl; i++) {
            const size_t n = (size_t)(ELE_PIXELS >> i) * (ELE_PIXELS >> i);
            e.pyr_laplace[i].resize(n * 3 * es); e.weights[i].resize(n);
            if (!pf_get_tile_level(h_, ix, iy, i, e.pyr_laplace[i].data(), e.weights[i].data())) return false;
        }
        return true;
    }
    bool blend(int ix, int iy, unsigned char* bgr256) { return pf_blend_tile(h_, ix, iy, bgr256) != 0; }
    // ... as the view of pyramid level `level`: BGR8 E x E, E = ELE_PIXELS >> level (pf_blend_tiles_level).  A tile without pyramid
    // leaves bgr untouched; false where the map has no such level
    bool blendLevel(int ix, int iy, int level, unsigned char* bgr)
    {
        const int xy[2] = { ix, iy };
        return pf_blend_tiles_level(h_, xy, 1, level, bgr, nullptr) != 0;
    }
    // save() without the file, at pyramid level `level` (0: the full mosaic): rows x cols x 3 BGR8 into `bgr`, the origin tile
    bool saveToMemory(std::vector<unsigned char>& bgr, int& rows, int& cols, int& tile_x0, int& tile_y0, int level = 0)
    {
        if (!pf_save_to_memory_level(h_, level, nullptr, &rows, &cols, &tile_x0, &tile_y0)) return false;
        bgr.resize((size_t)rows * cols * 3);
        return pf_save_to_memory_level(h_, level, bgr.data(), &rows, &cols, &tile_x0, &tile_y0) != 0;
    }
    // draw() at the operator's pan, zoom and rotation, without GL (pf_render_view): the mosaic under V -- row-major 3 x 3, plane metres ->
    // view pixels -- as height x width x channels bytes, B G R and with channels = 4 the coverage; level -1: the pyramid level the view's
    // scale chooses.  Rendered on the GPU from the tiles the view depends on.  Returns the image; empty, with the reason in
    // pf_last_error(), where the view is refused.  info (may be null): the plan
    std::vector<unsigned char> drawView(const double V[9], int width, int height, int level = -1, int channels = 4, pf_view_info* info = nullptr)
    {
        std::vector<unsigned char> image;
        if (width < 1 || height < 1 || (channels != 3 && channels != 4)) return image;
        image.resize((size_t)width * height * channels);
        if (!pf_render_view(h_, V, width, height, level, channels, image.data(), 0, info)) image.clear();
        return image;
    }
    // V of what the camera of prepare() sees at `pose` (camera to world); false for a pose feed() would reject
    template <class SE3> bool viewFromPose(const SE3& pose, double V[9])
    {
        double p[7];
        pifusion::pose7(pose, p);
        return pf_view_from_pose(h_, p, nullptr, V) != 0;
    }
    pf_map* handle() { return h_; }

private:
    explicit Map2D(pf_map* h) : h_(h) {}
    pf_map* h_;
    unsigned char* tex_ = nullptr; size_t tex_cap_ = 0;      // draw()'s page-locked tile buffer
    bool fuse2google_ = false;
    double gps_origin_[3] = { 0, 0, 0 };
};

#endif  // PIFUSION_MAP2D_H
