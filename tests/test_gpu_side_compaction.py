"""-m gpu: the ordered compaction that the quad finder and the chessboard finder share (csrc/agt_side_device.h: a count per chunk of
1024 elements, one workgroup's exclusive scan per frame in rounds of 256 chunks, the rank inside the chunk), at the smallest shapes
at which it can go wrong, each held to the numpy statement of the library's rule (tests/quad_detect_numpy.py,
tests/chessboard_numpy.py) with array_equal.  Every scene is first held to what it is built for -- where its roots or maxima lie --
so that a case cannot go empty unnoticed.

What the quad finder shows of an id: a component's id is its row of the support table, so two components with one id mix their
support points and the quad of either changes; and with max_components = k exactly the k first kept roots are examined, so a quad
whose root is the k-th kept one comes and goes with the cap."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import chessboard_numpy as cb       # noqa: E402
import quad_detect_numpy as qd      # noqa: E402
from test_gpu_chessboard import texture         # noqa: E402
from test_gpu_quad_detect import device_detect  # noqa: E402

pytestmark = pytest.mark.gpu

CHUNK = 1024                        # elements per workgroup of the count and rank kernels: 4 iterations of 256 threads, waves of 64


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("needs a GPU")
    torch.cuda.set_device(0)
    return torch


def equal(got, want, what):
    for name, g, w in zip(("first", "second", "third"), got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, name)


def roots(frame, **kw):
    lab = qd.labels(frame, **kw)
    return np.nonzero(lab.reshape(-1) == np.arange(lab.size))[0].tolist()


def white(h, w, dark_pixels=(), squares=()):
    """a white frame with single dark pixels at linear indices and dark squares (x, y, side)"""
    f = np.full((h, w), 255, np.uint8)
    f.reshape(-1)[list(dark_pixels)] = 0
    for x, y, s in squares:
        f[y:y + s, x:x + s] = 0
    return f


# ---- the quad finder

SEAM_W, SEAM_H = 41, 25             # 1025 pixels: the second chunk holds one
SEAM_SQUARE = (14, 10, 10)          # rooted at pixel 10 * 41 + 14 = 424, behind both wave seams
SEAM_HELP = 22 * 41 + 36            # a dark pixel inside the last whole tile row: pixels of row 24 and column 40 take their threshold
#                                     from the tiles of rows 20..23 and columns 36..39, which need contrast of their own
# Dark pixels next to each other in a row are ONE component, so roots cannot sit at 63 and 64 (or 1023 and 1024) of one frame: frame
# 0 has them at the odd indices -- 63, 255 and 1023: the last lane before each seam -- and frame 1 at the even ones -- 64, 256 and
# 1024: the first lane behind it, 1024 being the one pixel of the second chunk.
SEAM_ROOTS = [[59, 61, 63, 65, 67, 251, 253, 255, 257, 259, 1021, 1023], [60, 62, 64, 66, 252, 254, 256, 258, 1020, 1022, 1024]]


def seam_frames():
    return np.stack([white(SEAM_H, SEAM_W, r + [SEAM_HELP], [SEAM_SQUARE]) for r in SEAM_ROOTS])


def test_quad_ids_at_the_one_pixel_tail_and_the_wave_seams(torch_cuda):
    """41 x 25, B = 2, min_area = 1: roots on both sides of lanes 63|64, of the iterations' seam 255|256 and of the chunks' seam
    1023|1024, a quad rooted between them.  With every root in the table, and with the cap at the quad's id + 1 (it is the last
    component examined) and at its id (it is left out)."""
    frames = seam_frames()
    square_root = SEAM_SQUARE[1] * SEAM_W + SEAM_SQUARE[0]
    for f, want_roots in zip(frames, SEAM_ROOTS):
        assert roots(f) == sorted(want_roots + [square_root, SEAM_HELP])
    ids = [sorted(r + [square_root]).index(square_root) for r in SEAM_ROOTS]
    assert ids == [10, 8]
    for cap, found in ((4096, [1, 1]), (11, [1, 1]), (10, [0, 1]), (8, [0, 0])):
        got = device_detect(torch_cuda, frames, max_components=cap, max_quads=4, min_area=1)
        want = qd.detect_batch(frames, max_components=cap, max_quads=4, min_area=1)
        equal(got, want, "cap %d" % cap)
        assert want[2][:, 1].tolist() == [len(r) + 2 for r in SEAM_ROOTS] == [14, 13] and want[2][:, 2].tolist() == found, (cap, want[2].tolist())
        assert [int(v) for v in want[1]["label"][:, 0]] == [square_root * n for n in found]


def test_quad_ids_in_the_second_round_of_the_scan(torch_cuda):
    """513 x 512: 257 chunks, so the scan's second round holds one chunk, which is row 511 from x = 1 on.  Quads in the first rows, the
    first of them the component with id 0, and a dark run in row 511 whose root lies in that last chunk: an id that does not carry
    the first round's total would land in a quad's row of the support table and move its lowest point.  Counts, the ordered quads and
    records and the zeroed rest behind them."""
    w, h = 513, 512
    f = white(h, w, squares=[(6, 3, 12), (40, 5, 9), (300, 8, 16), (100, 400, 20)])
    f[511, 200:206] = 0
    f[509, 210] = 0                 # (contrast for row 511's tiles, as in the seam scene)
    r = roots(f)
    assert r[0] == 3 * w + 6 and r[-1] == 511 * w + 200 and r[-1] // CHUNK == 256 and (w * h + CHUNK - 1) // CHUNK == 257
    got = device_detect(torch_cuda, f[None], max_quads=8, min_area=1)
    want = qd.detect_batch(f[None], max_quads=8, min_area=1)
    equal(got, want, "513 x 512")
    assert want[2][0].tolist() == [6, 6, 4, 0] and not want[0][0, 4:].any() and not want[1][0, 4:].view(np.uint8).any()
    # ... and with the cap at the last root's id: it is the one left out, the quads stay
    got = device_detect(torch_cuda, f[None], max_components=5, max_quads=5, min_area=1)
    want = qd.detect_batch(f[None], max_components=5, max_quads=5, min_area=1)
    equal(got, want, "513 x 512, max_components 5")
    assert want[2][0].tolist() == [6, 6, 4, qd.FLAG_COMPONENTS]


def test_quad_ids_on_a_workspace_used_for_a_larger_frame(torch_cuda):
    """a handle for 256 x 160 (40 chunks a frame, B = 2) first used at that size on a frame of some thousand roots, then at 41 x 25
    (two chunks a frame, laid out [B][2] for this call) with the cap under the kept count: the larger call's chunk counts are
    nobody's"""
    from accurate_aprilgroup_tracking_amd import quad_detect
    det = quad_detect.QuadDetector(256, 160, max_batch=2, max_components=9, max_quads=4)
    big = np.full((2, 160, 256), 255, np.uint8)
    big[:, 1::2, 1::2] = 0                                  # a dark pixel in every 2 x 2 cell: 80 x 128 one-pixel components
    got = device_detect(torch_cuda, big, detector=det, min_area=1)
    want = qd.detect_batch(big, max_components=9, max_quads=4, min_area=1)
    equal(got, want, "256 x 160")
    assert want[2][:, :2].tolist() == [[80 * 128] * 2] * 2 and want[2][:, 3].tolist() == [qd.FLAG_COMPONENTS] * 2
    frames = seam_frames()
    want = qd.detect_batch(frames, max_components=9, max_quads=4, min_area=1)
    assert want[2].tolist() == [[14, 14, 0, qd.FLAG_COMPONENTS], [13, 13, 1, qd.FLAG_COMPONENTS]]      # (the quad's ids are 10 and 8)
    for note in ("first", "again"):
        equal(device_detect(torch_cuda, frames, detector=det, min_area=1), want, "41 x 25 after 256 x 160, " + note)


# ---- the chessboard finder: the candidates' table is the compaction's own output, in raster order

def device_candidates(torch, frames, max_candidates, finder=None, **options):
    from accurate_aprilgroup_tracking_amd import chessboard
    f = torch.from_numpy(np.array(frames)).cuda()
    if finder is None:
        finder = chessboard.ChessboardFinder(f.shape[2], f.shape[1], f.shape[0], max_candidates)
    table, counts = finder.candidates(f, **options)
    torch.cuda.synchronize()
    return table.cpu().numpy(), counts.cpu().numpy()


def statement_candidates(frames, max_candidates, **options):
    parts = [cb.candidates(cb.response(f), max_candidates, **options) for f in frames]
    return tuple(np.stack([p[k] for p in parts]) for k in range(2))


LOW = dict(min_response=1, rel_pct=0, nms=1)        # every positive 3 x 3 maximum of the response is a candidate


def SEAM_TEXTURES():
    return np.stack([texture(37, 64, 9), texture(37, 64, 26), texture(37, 64, 10, smooth=False)])


def test_chess_ids_at_the_wave_iteration_and_chunk_seams(torch_cuda):
    """64 x 37: a row is a wave, four rows an iteration, 16 rows a chunk, and the third chunk is partly filled (5 rows, none of which
    has a response).  Random frames at the lowest thresholds -- two smoothed ones with some thirty maxima, a rough one with some seventy --
    with candidates in rows 7 | 8 (an iterations' seam), 15 | 16 (the chunks' seam) and 31 (the last row with a response), each row
    another wave.  All of them, and with the cap inside the second chunk."""
    w, h = 64, 37
    frames = SEAM_TEXTURES()
    full = statement_candidates(frames, 1024, **LOW)
    for table, counts in zip(*full):
        rows = set(table[:counts[1], 1].tolist())
        assert counts[0] == counts[1] and {7, 8, 15, 16, 31} <= rows and max(rows) == h - 6, sorted(rows)
    assert full[1][2, 1] > 60
    equal(device_candidates(torch_cuda, frames, 1024, **LOW), full, "64 x 37")
    cap = int(min((t[:n[1], 1] < 20).sum() for t, n in zip(*full)))
    cut = statement_candidates(frames, cap, **LOW)
    assert np.all(cut[1][:, 0] > cap) and cut[1][:, 1].tolist() == [cap] * 3 and cut[1][:, 3].tolist() == [cb.FLAG_CANDIDATES] * 3
    equal(device_candidates(torch_cuda, frames, cap, **LOW), cut, "64 x 37, cap %d" % cap)


@pytest.mark.parametrize("w,h", [(513, 512), (1024, 263)])
def test_chess_ids_in_the_second_round_of_the_scan(torch_cuda, w, h):
    """513 x 512: 257 chunks; the last one is row 511, inside the border that has no response, so the scan's second round holds a
    count of zero behind the total of the first.  1024 x 263: a chunk is a row, 263 chunks, and rows 256 and 257 hold maxima, whose ids
    start at the first round's total.  Texture in the first rows and in the last ones that can respond, a flat frame between (no
    response: the statement stays cheap); counts, the table in raster order and its zeroed rest."""
    f = np.full((h, w), 128, np.uint8)
    f[:24] = texture(24, w, 21)
    f[h - 24:] = texture(24, w, 22)
    want = statement_candidates(f[None], 2048, **LOW)
    n = int(want[1][0, 1])
    ys = want[0][0, :n, 1]
    assert want[1][0, 0] == n < 2048 and (ys < 24).sum() > 3 and ys.max() == h - 6 and not want[0][0, n:].any()
    assert (w * h + CHUNK - 1) // CHUNK > 256 and (h == 512 or ((ys * w + want[0][0, :n, 0]) // CHUNK >= 256).sum() > 3)
    equal(device_candidates(torch_cuda, f[None], 2048, **LOW), want, "%d x %d" % (w, h))


def test_chess_ids_on_a_workspace_used_for_a_larger_frame(torch_cuda):
    """a finder for 256 x 160 (40 chunks a frame) first used at that size with B = 2, then at 64 x 37 (three chunks a frame) with
    B = 3 and the cap under the candidates' count, twice"""
    from accurate_aprilgroup_tracking_amd import chessboard
    fd = chessboard.ChessboardFinder(256, 160, 3, 20)
    big = np.stack([texture(160, 256, seed) for seed in (31, 32)])
    want = statement_candidates(big, 20, **LOW)
    assert np.all(want[1][:, 0] > 500)
    equal(device_candidates(torch_cuda, big, 20, finder=fd, **LOW), want, "256 x 160")
    frames = SEAM_TEXTURES()
    want = statement_candidates(frames, 20, **LOW)
    assert np.all(want[1][:, 0] > 20) and want[1][:, 3].tolist() == [cb.FLAG_CANDIDATES] * 3
    for note in ("first", "again"):
        equal(device_candidates(torch_cuda, frames, 20, finder=fd, **LOW), want, "64 x 37 after 256 x 160, " + note)
