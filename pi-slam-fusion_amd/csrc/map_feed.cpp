// map_feed.cpp -- the way into the map (fusion_map.hpp): prepare, frame slots and uploads, the input camera, feed, the frame
// distribution hooks, the worker thread and sync, following Map2D.cpp and MultiBandMap2DCPU.cpp:199-309, :606-635.
#include "fusion_map.hpp"
#include "map_internal.hpp"
#include "warp_index.hpp"
#include "raw_convert.hpp"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>

namespace pf {

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
    if (und_set_) { und_table_ = std::move(und_table); und_uncovered_ = und_uncovered; }
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
        (void)hipGetLastError(); set_error("input camera: upload of the remap table failed"); return false;
    }
    buf = std::move(b);
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
    und_set_ = n != 0; und_cam_ = cam; und_table_ = std::move(table); und_uncovered_ = unc;
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

// ---- raw frames (raw_convert.hpp, raw_convert.hip): a front end in the line of pf_feed_jpeg and the input camera
// The producer of a raw keyframe.  dst: the slot feed() or undistort_frame() acquired for the BGR8 picture.  Host planes go, as they lie,
// into one scratch slot by a blocking copy each -- the caller may release them when the feed returns -- and the kernel reads them there.
bool FusionMap::produce_raw(const pf_raw_frame& src, bool device_planes, uint8_t* dst, hipStream_t st)
{
    pf_raw_frame dev = src;
    int scratch = -1;
    if (!device_planes) {
        const int np = raw::planes_of(src.format);
        size_t off[3] = { 0, 0, 0 }, total = 0;
        for (int k = 0; k < np; k++) { off[k] = total; total += (raw::plane_bytes(src, k) + 255) & ~(size_t)255; }
        // dst's slot is acquired but neither queued nor pending yet: held, so that it is not handed out a second time as the scratch slot
        int own = -1;
        for (size_t i = 0; i < slots_.size(); i++) if (slots_[i].dev == dst) own = (int)i;
        if (own >= 0) { std::lock_guard<std::mutex> q(qmu_); slots_[own].queued = true; }
        scratch = acquire_slot(total);
        if (own >= 0) { std::lock_guard<std::mutex> q(qmu_); slots_[own].queued = false; }
        if (scratch < 0) return false;
        for (int k = 0; k < np; k++) {
            HIP_OK(hipMemcpy(slots_[scratch].dev + off[k], src.plane[k], raw::plane_bytes(src, k), hipMemcpyHostToDevice));
            dev.plane[k] = slots_[scratch].dev + off[k];
        }
    }
    launch_raw_convert(st, dev, dst, (size_t)src.cols * 3);
    const hipError_t e = hipGetLastError();
    // the scratch slot's next blocking upload has to wait for the kernel that reads it
    if (scratch >= 0) slots_[scratch].pending = hipEventRecord(slots_[scratch].consumed, st) == hipSuccess;
    if (e != hipSuccess) { set_error(std::string("raw conversion: ") + hipGetErrorString(e)); return false; }
    if (scratch >= 0 && !slots_[scratch].pending) { set_error("feed: hipEventRecord failed"); return false; }
    return true;
}

bool FusionMap::feed_raw(const pf_raw_frame* src, const double pose7[7], bool device_planes)
{
    const char* who = device_planes ? "pf_feed_raw_device: " : "pf_feed_raw: ";
    std::string why;
    if (!src || !pose7) { set_error(std::string(who) + "no frame or no pose"); return false; }
    if (!raw::check(*src, why)) { set_error(who + why); return false; }
    if (device_planes && thread_) { set_error("pf_feed_raw_device needs a thread=0 map"); return false; }
    // from here on a BGR8 frame of the raw frame's size whose pixels the producer writes: size gate, counters, queue, lookahead as feed() has them
    const pf_image desc{ src->rows, src->cols, PF_8UC3, nullptr, 0 };
    const FrameProducer fill = [this, src, device_planes](void* dev, hipStream_t st) { return produce_raw(*src, device_planes, (uint8_t*)dev, st); };
    return feed(&desc, pose7, false, &fill);
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
    prof_.harvest();
    if (lost) { set_error(fail_msg_); return false; }
    return drained;
}

}  // namespace pf
