// The level-view members of the header-only C++ face (include/pifusion/Map2D.h): compiled with -fsyntax-only by
// tests/test_level_view_model.py, never run.
#include <pifusion/Map2D.h>
#include <cstdio>
#include <vector>

int main()
{
    std::shared_ptr<Map2D> map = Map2D::create(Map2D::TypeMultiBandCPU, false);
    if (!map) return 0;
    const int level = 2, e = ELE_PIXELS >> level;
    int refreshed = 0;
    map->drawLevel(level, [&](int, int, const unsigned char* bgr) { refreshed += bgr != nullptr; });
    std::vector<unsigned char> tile((size_t)e * e * 3), mosaic;
    const bool blended = map->blendLevel(0, 0, level, tile.data());
    int rows = 0, cols = 0, tx0 = 0, ty0 = 0;
    const bool saved = map->saveToMemory(mosaic, rows, cols, tx0, ty0, level);
    std::printf("%d %d %d %d x %d at (%d, %d)\n", refreshed, (int)blended, (int)saved, rows, cols, tx0, ty0);
    // the C entry points themselves
    int xy[2] = { 0, 0 };
    (void)pf_blend_tiles_level(map->handle(), xy, 1, level, tile.data(), nullptr);
    (void)pf_blend_changed_level(map->handle(), level, xy, tile.data(), 1);
    (void)pf_save_to_memory_level(map->handle(), level, nullptr, &rows, &cols, &tx0, &ty0);
    return 0;
}
