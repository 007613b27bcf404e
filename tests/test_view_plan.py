"""The plan of a rendered view (pi-slam-fusion_amd/csrc/view_plan.hpp behind pf_view_plan -- the very code the engine runs) against numpy
written out longhand: A_k and M0 to the last bit, Minv against the oracle's closed form, the automatic level on both sides of every
power of two, the rectangle of tiles against a brute-force dependency model of the collapse, the structural claim (the tiles collapsed
depend on the view, not on the extent) and every refusal.  No device, no map.  (The helpers that make a V need a map, and a map needs a
device: they are checked in tests/test_gpu_view.py.)"""
import numpy as np
import pytest

ELE = 256
# a dyadic grid: every product below is exact, so a boundary that is meant to be hit is hit
LP, ELE_SIZE = 0.25, 64.0
DIMS = [50, 50, 3, 2]                        # w, h, off_x, off_y
GEO = [-64.0, -32.0, 3136.0, 3168.0, ELE_SIZE, LP]


def level_to_plane(k, tx, ty, dims=DIMS, geo=GEO):
    s = geo[5] * float(1 << k)
    return [[s, 0.0, geo[0] + (tx - dims[2]) * geo[4]], [0.0, s, geo[1] + (ty - dims[3]) * geo[4]], [0.0, 0.0, 1.0]]


def triple_loop(P, Q):
    R = [[0.0] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(3):
            s = 0.0
            for k in range(3):
                s = s + float(P[i][k]) * float(Q[k][j])
            R[i][j] = s
    return R


def crop_view(k, extent, ax, ay):
    """V of scale 1 at level k: view pixel (u, v) lies over level-k pixel (u + ax, v + ay) of the extent.  Exact on the dyadic grid"""
    A = level_to_plane(k, extent[0], extent[1])
    s, ox, oy = A[0][0], A[0][2], A[1][2]
    return np.array([[1 / s, 0, -ox / s - ax], [0, 1 / s, -oy / s - ay], [0, 0, 1.0]])


def random_views(n, seed):
    rng = np.random.RandomState(seed)
    for _ in range(n):
        a = rng.uniform(-np.pi, np.pi); s = 2.0 ** rng.uniform(-2, 3)
        V = np.array([[s * np.cos(a), -s * np.sin(a), 0.0], [s * np.sin(a), s * np.cos(a), 0.0], [rng.uniform(-1e-4, 1e-4), rng.uniform(-1e-4, 1e-4), 1.0]])
        # a plane point of the tests' extents (metres) goes to about the middle of the view
        c = np.array([rng.uniform(100, 400), rng.uniform(120, 400), 1.0])
        p = V @ c
        V[0, 2] = 40 * p[2] - p[0]; V[1, 2] = 20 * p[2] - p[1]
        yield V


def test_matrices_to_the_last_bit(pf, orc):
    extent = (5, 4, 6, 5)
    seen = 0
    for V in random_views(40, 1):
        for level in (0, 2, 5):
            try:
                info = pf.view_plan(V, 150, 37, level, DIMS, GEO, 6, extent)
            except ValueError:
                continue
            if info["empty"]:
                continue
            seen += 1
            tx, ty = info["rect"][:2]
            M0 = np.array(triple_loop(V, level_to_plane(level, tx, ty)))
            assert info["M0"].tobytes() == M0.tobytes(), (level, info["M0"] - M0)
            assert info["Minv"].tobytes() == orc.invert3x3(M0).tobytes()
            assert info["tiles"] == info["rect"][2] * info["rect"][3] and info["level"] == level
    assert seen >= 30


@pytest.mark.parametrize("L", [0, 3, 5, 8])
def test_automatic_level_on_both_sides_of_every_power_of_two(pf, L):
    """V = diag(1 / (lp s)): one view pixel spans s level-0 pixels.  s = 2^j exactly belongs to level j, a millionth below it to j - 1"""
    extent = (3, 2, 4, 4)
    for j in range(0, 11):
        for s, want in ((2.0 ** j, j), (2.0 ** j * (1 + 2.0 ** -20), j), (2.0 ** j / (1 + 2.0 ** -20), j - 1)):
            V = np.diag([1 / (LP * s), 1 / (LP * s), 1.0])
            V[0, 2], V[1, 2] = 7.0, -3.0
            info = pf.view_plan(V, 64, 48, -1, DIMS, GEO, L + 1, extent)
            assert info["level"] == min(max(want, 0), L), (j, s)
    # magnified views stay at level 0; a rotation and a flip do not change the scale
    assert pf.view_plan(np.diag([64.0, 64.0, 1.0]), 64, 48, -1, DIMS, GEO, L + 1, extent)["level"] == 0
    c = 1 / (LP * 4.0)
    assert pf.view_plan(np.array([[0, -c, 5], [c, 0, 9], [0, 0, 1.0]]), 64, 48, -1, DIMS, GEO, L + 1, extent)["level"] == min(2, L)
    assert pf.view_plan(np.array([[-c, 0, 5], [0, c, 9], [0, 0, 1.0]]), 64, 48, -1, DIMS, GEO, L + 1, extent)["level"] == min(2, L)


def brute_force_tiles(lo, hi, k, L, n_tiles):
    """tiles (an inclusive range) that the level-k pixels lo .. hi of an image n_tiles tiles long depend on: the window marked in an array
    of booleans at level k and the dependence pushed up level by level with pyrUp's 3-tap rule -- an even pixel 2 s reads s - 1, s, s + 1,
    an odd one 2 s + 1 reads s, s + 1; past the image's ends pyrUp reads pixels inside it"""
    need = np.zeros(n_tiles * (ELE >> k), bool)
    need[lo:hi + 1] = True
    tiles = set(np.flatnonzero(need) // (ELE >> k))
    for i in range(k + 1, L + 1):
        n = n_tiles * (ELE >> i)
        up = np.zeros(n, bool)
        for x in np.flatnonzero(need):
            s = x >> 1
            for t in ((s - 1, s, s + 1) if x % 2 == 0 else (s, s + 1)):
                up[min(max(t, 0), n - 1)] = True
        need = up
        tiles |= set(np.flatnonzero(need) // (ELE >> i))
    return min(tiles), max(tiles)


@pytest.mark.parametrize("L", [0, 1, 5, 8])
def test_rectangle_against_a_brute_force_dependency_model(pf, L):
    ex = (7, 9, 6, 5)                       # first tile, tiles across and down
    for k in range(L + 1):
        e = ELE >> k
        cols, rows = ex[2] * e, ex[3] * e
        # windows of level-k pixels [a, b]: on a tile border, a pixel inside it, a pixel before it, at the extent's edges, across them
        starts = sorted({0, 1, e, e + 1, 2 * e - 1, 2 * e, cols - 2, cols - 1, -3})
        ends = sorted({0, e - 1, e, 2 * e - 1, 2 * e, 3 * e - 2, cols - 2, cols - 1, cols + 4})
        cases = [(a, b) for a in starts for b in ends if b >= a and b - a < 16384 and b >= 0 and a <= cols - 1]
        assert len(cases) > 10 or e <= 2
        for n, (a, b) in enumerate(cases):
            # the view's pixels u = 0 .. b - a - 1 lie over level-k pixels a .. b - 1; the second tap makes the window a .. b
            width = max(b - a, 1)
            ay = (n * 37) % max(rows - 3, 1)
            V = crop_view(k, ex, a, ay)
            info = pf.view_plan(V, width, 3, k, DIMS, GEO, L + 1, ex)
            lo, hi = max(a, 0), min(a + width, cols - 1)
            ylo, yhi = ay, min(ay + 3, rows - 1)
            assert not info["empty"], (k, a, b)
            tx, ty, nx, ny = info["rect"]
            assert info["window"] == (lo - (tx - ex[0]) * e, ylo - (ty - ex[1]) * e, hi - lo + 1, yhi - ylo + 1), (k, a, b, info)
            bx = brute_force_tiles(lo, hi, k, L, ex[2]); by = brute_force_tiles(ylo, yhi, k, L, ex[3])
            assert (tx - ex[0], tx - ex[0] + nx - 1) == bx and (ty - ex[1], ty - ex[1] + ny - 1) == by, (L, k, a, b, info["rect"], bx, by)
            assert info["tiles"] == nx * ny
            # the same window through the rows
            ext = (ex[0], ex[1], ex[3], ex[2])
            info_t = pf.view_plan(crop_view(k, ext, ay, a), 3, width, k, DIMS, GEO, L + 1, ext)
            assert info_t["rect"] == (ex[0] + by[0], ex[1] + bx[0], ny, nx), (L, k, a, b, info_t["rect"])


def test_eight_bands_need_two_tiles_of_ring():
    """where the top level is one pixel a tile, a window on a tile's last column (with the pixel behind it for the second tap) depends
    on TWO tiles to its right -- pyrUp reaches one pixel further up at every level, and at the top a pixel is a tile --, one on its
    first column on one tile to either side; with five bands one tile of ring is enough.  The brute-force model says so by itself"""
    assert brute_force_tiles(3 * ELE, 3 * ELE + 1, 0, 8, 8) == (2, 4)
    assert brute_force_tiles(4 * ELE - 1, 4 * ELE, 0, 8, 8) == (3, 5)
    assert brute_force_tiles(3 * ELE, 3 * ELE + 1, 0, 5, 8) == (2, 3)
    assert brute_force_tiles(4 * ELE - 1, 4 * ELE, 0, 5, 8) == (3, 4)


@pytest.mark.parametrize("L,small", [(5, 3), (8, 7)])
def test_tiles_depend_on_the_view_not_on_the_extent(pf, L, small):
    """the same views over a small extent and over one of 40 x 40 tiles that holds it: the same tiles are collapsed"""
    a = (20 - small // 2, 20 - small // 2, small, small)
    b = (0, 0, 40, 40)
    mid = ((a[0] + small // 2) - DIMS[2]) * ELE_SIZE + GEO[0], ((a[1] + small // 2) - DIMS[3]) * ELE_SIZE + GEO[1]          # the middle tile's corner, metres
    n = 0
    for V0 in random_views(12, 5):
        V = V0.copy(); V[2, :2] = 0
        # centre the view on the middle tile
        c = V @ np.array([mid[0] + ELE_SIZE / 2, mid[1] + ELE_SIZE / 2, 1.0])
        V[0, 2] += 32 - c[0]; V[1, 2] += 32 - c[1]
        for level in (-1, 0, min(3, L)):
            ia = pf.view_plan(V, 64, 64, level, DIMS, GEO, L + 1, a)
            ib = pf.view_plan(V, 64, 64, level, DIMS, GEO, L + 1, b)
            if ia["rect"][2] == small or ia["rect"][3] == small:
                continue                     # the small extent cut the ring: not the same question
            n += 1
            assert ia["tiles"] == ib["tiles"] and ia["rect"] == ib["rect"] and ia["level"] == ib["level"], (level, ia, ib)
            assert ia["M0"].tobytes() == ib["M0"].tobytes()
    assert n >= 12


def refused(pf, V, width=64, height=48, level=0, extent=(3, 2, 4, 4), levels=6, word=None):
    import ctypes as C
    info = pf.ViewInfo(); info.level = 77; info.tiles = 77
    a = np.ascontiguousarray(V, np.float64).reshape(9)
    ok = pf.lib().pf_view_plan(a.ctypes.data_as(C.POINTER(C.c_double)), width, height, level, (C.c_int * 4)(*DIMS), (C.c_double * 6)(*GEO), levels,
                               (C.c_int * 4)(*extent), C.byref(info))
    msg = pf.lib().pf_last_error().decode()
    assert ok == 0 and msg.startswith("pf_view_plan: ") and (word is None or word in msg), (ok, msg)
    assert info.level == 77 and info.tiles == 77, "a refusal wrote its result"
    return msg


def test_refusals_name_the_reason_and_write_nothing(pf):
    I = crop_view(0, (3, 2, 4, 4), 10, 10)
    assert not pf.view_plan(I, 64, 48, 0, DIMS, GEO, 6, (3, 2, 4, 4))["empty"]
    for bad in (np.nan, np.inf, -np.inf):
        for i in range(9):
            V = I.copy(); V.reshape(9)[i] = bad
            refused(pf, V, word="finite")
    refused(pf, np.zeros((3, 3)), word="singular")
    refused(pf, np.array([[1, 2, 3], [2, 4, 6], [0, 0, 1.0]]), word="singular")
    for w, h in ((0, 48), (64, 0), (-1, 48), (16385, 48), (64, 16385)):
        refused(pf, I, width=w, height=h, word="16384")
    assert pf.view_plan(I, 16384, 1, 0, DIMS, GEO, 6, (3, 2, 4, 4))["level"] == 0
    for level in (-2, 6, 9):
        refused(pf, I, level=level, word="level")
    # the horizon inside the view: the denominator of (view pixel -> level pixel) changes sign between two corners, along x and along y
    A0 = np.array(level_to_plane(0, 3, 2))
    for row in ([-2.0 / 63, 0, 1.0], [0, -2.0 / 47, 1.0], [-2.0 / 63, -2.0 / 47, 1.0], [0, -1.0 / 47, 1.0]):
        Minv = np.array([[1.0, 0, 10], [0, 1.0, 10], row])
        V = np.linalg.inv(Minv) @ np.linalg.inv(A0)
        if row[1] == -1.0 / 47 and row[0] == 0:
            Minv_check = np.linalg.inv(V @ A0)
            if (Minv_check[2] @ np.array([0, 47, 1.0])) * Minv_check[2, 2] > 0:
                continue                     # rounding left the zero on the near side: not the case meant
        refused(pf, V, word="horizon")
    # a mild perspective whose denominator keeps its sign is a view like any other
    Minv = np.array([[1.0, 0, 10], [0, 1.0, 10], [0.5 / 63, 0.2 / 47, 1.0]])
    assert not pf.view_plan(np.linalg.inv(Minv) @ np.linalg.inv(A0), 64, 48, 0, DIMS, GEO, 6, (3, 2, 4, 4))["empty"]
    # more than 32767 level-k pixels a side: refused at the level given, and the message says what to do; the automatic level fits
    wide = (0, 0, 200, 3)
    V = crop_view(0, wide, 0, 0); V[:2] /= 50.0          # one view pixel spans 50 level-0 pixels
    msg = refused(pf, V, width=1024, height=8, level=0, extent=wide, word="32767")
    assert "higher level" in msg
    info = pf.view_plan(V, 1024, 8, -1, DIMS, GEO, 6, wide)
    assert info["level"] == 5 and info["rect"][2] * (ELE >> 5) <= 32767 and not info["empty"]


def test_a_view_beside_the_extent_or_of_an_empty_map_is_empty(pf):
    ex = (3, 2, 4, 4)
    for ax, ay in ((-500, 10), (10, -500), (4 * ELE + 1, 10), (10, 4 * ELE + 1), (-65, 0), (0, -49)):
        info = pf.view_plan(crop_view(0, ex, ax, ay), 64, 48, 0, DIMS, GEO, 6, ex)
        assert info["empty"] and info["tiles"] == 0 and info["rect"] == (0, 0, 0, 0) and info["level"] == 0, (ax, ay, info)
    # one pixel nearer, a tap reaches the extent's first or last pixel
    for ax, ay in ((-64, 0), (0, -48), (4 * ELE - 1, 10), (10, 4 * ELE - 1)):
        assert not pf.view_plan(crop_view(0, ex, ax, ay), 64, 48, 0, DIMS, GEO, 6, ex)["empty"], (ax, ay)
    for none in ((0, 0, 0, 0), (3, 2, 0, 4), (3, 2, 4, 0)):
        info = pf.view_plan(crop_view(0, ex, 5, 5), 64, 48, -1, DIMS, GEO, 6, none)
        assert info["empty"] and info["tiles"] == 0
    # what is refused with content is refused without
    refused(pf, np.zeros((3, 3)), extent=(0, 0, 0, 0), word="singular")
