// Compiles Map2D::savePng of the C++ face (include/pifusion/Map2D.h) against libpifusion.so: both forms of the call, on a box without a
// device (create() returns null: nothing to save) and on a GPU (a small map saved as RGB and as RGBA; the files begin with the PNG
// signature and differ in the colour type).
#include <pifusion/Map2D.h>
#include <cstdio>
#include <string>
#include <vector>

static int colour_type(const std::string& path)
{
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) return -1;
    unsigned char h[26];
    const size_t n = std::fread(h, 1, sizeof h, f);
    std::fclose(f);
    return n == sizeof h && h[0] == 0x89 && h[1] == 'P' && h[2] == 'N' && h[3] == 'G' ? h[25] : -1;
}

int main(int argc, char** argv)
{
    bool (Map2D::*member)(const std::string&, bool) = &Map2D::savePng;          // the declared signature
    (void)member;
    std::shared_ptr<Map2D> map = Map2D::create(Map2D::TypeMultiBandCPU, false);
    if (!map) { std::printf("no device: create() returned null\n"); return 0; }
    const std::string dir = argc > 1 ? argv[1] : ".";
    std::vector<unsigned char> px(480 * 640 * 3, 90);
    pifusion::ImageView img(480, 640, PF_8UC3, px.data());
    std::deque<std::pair<pifusion::ImageView, pi::SE3d>> frames;
    for (int k = 0; k < 3; k++) frames.push_back(std::make_pair(img, pi::SE3d(10. * k, 0, -100, 0, 0, 0, 1)));
    if (!map->prepare(pi::SE3d(), PinHoleParameters(640, 480, 500, 500, 320, 240), frames)) return 3;
    for (auto& f : frames) if (!map->feed(f.first, f.second)) return 4;
    if (!map->savePng(dir + "/rgb.png") || !map->savePng(dir + "/rgba.png", true)) return 5;
    if (colour_type(dir + "/rgb.png") != 2 || colour_type(dir + "/rgba.png") != 6) return 6;
    if (map->savePng(dir + "/missing/x.png")) return 7;
    std::printf("png files written\n");
    return 0;
}
