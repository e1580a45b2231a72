"""CPU: the tag decode library (include/agt_tagcode.h -> libagt_tagcode.so) builds, exports exactly its header, keeps its kernel out
of scratch and judges its arguments without a device; the numpy statement of the rule (tests/tag_decode_numpy.py) that the GPU tests
compare with reads the rendered truth without a bit error, and has the properties the rule promises; the host parts (family
generator, family file)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import tag_decode_numpy as tn      # noqa: E402
import tag_decode_scenes as ts     # noqa: E402

from accurate_aprilgroup_tracking_amd import synthetic as syn    # noqa: E402

# a tag's margin is half its local contrast (97.5 for the renderer's 30 / 225), bare background stays under 15: 30 lies between with
# a factor of two to either side
MARGIN_GATE = 30.0


@pytest.fixture(scope="module")
def cand():
    return tn.candidates(ts.family_codes())


def test_tagcode_library_builds_exports_and_resources():
    import side_library
    from accurate_aprilgroup_tracking_amd import tagcodelib
    rows = side_library.built(tagcodelib, "tagcode")
    assert [re.search(r"(tag_\w+)\(", r["name"]).group(1) for r in rows] == ["tag_decode_kernel"]
    # no private segment, and room for four waves per SIMD
    bad = [(r["name"], r["scratch"], r["vgpr"], r["vspill"]) for r in rows if r["scratch"] != 0 or r["vgpr"] > 128 or r["vspill"] != 0]
    assert not bad, bad
    assert tagcodelib.lib().agt_tagcode_version() == tagcodelib.VERSION == 100
    assert tagcodelib.RECORD_DTYPE == tn.RECORD_DTYPE


def test_argument_errors_need_no_device():
    from accurate_aprilgroup_tracking_amd import tagcodelib as T
    L = T.lib()
    h = ctypes.c_void_p()
    codes = np.arange(1, 5, dtype=np.uint64)

    def create(c, n, bits=6, out=h):
        rc = L.agt_tag_family_create(None if c is None else c.ctypes.data, n, bits, None, None if out is None else ctypes.byref(out))
        assert not h.value
        return rc
    assert create(codes, 4, out=None) == T.ERR_ARG
    assert create(None, 4) == T.ERR_ARG
    assert create(codes, 0) == T.ERR_ARG
    assert create(codes, T.MAX_CODES + 1) == T.ERR_ARG
    for bits in (5, 7, 0):
        assert create(codes, 4, bits) == T.ERR_ARG
    high = codes.copy(); high[3] = np.uint64(1) << np.uint64(36)
    assert create(high, 4) == T.ERR_ARG
    assert L.agt_tag_family_destroy(None) == 0

    # agt_tag_decode: the family handle is judged last, so every other refusal shows without one; no pointer is followed
    good = dict(frames=64, pitch=640, frame_stride=640 * 480, width=640, height=480, B=2, quads=64, Q=12, max_hamming=2, min_margin=0.0, records=64)

    def decode(**kw):
        a = dict(good, **kw)
        return L.agt_tag_decode(None, a["frames"], a["pitch"], a["frame_stride"], a["width"], a["height"], a["B"], a["quads"], None, a["Q"], None,
                                a["max_hamming"], a["min_margin"], a["records"], None, None, None)
    assert decode() == T.ERR_FAMILY
    for k in ("frames", "quads", "records"):
        assert decode(**{k: None}) == T.ERR_ARG, k
    for kw in (dict(width=3), dict(height=3), dict(width=T.MAX_SIZE + 1, pitch=1 << 20, frame_stride=1 << 40), dict(height=T.MAX_SIZE + 1, frame_stride=1 << 40),
               dict(pitch=639), dict(frame_stride=640 * 479 + 639), dict(B=0), dict(Q=0), dict(B=-1), dict(B=1 << 10, Q=(1 << 10) + 1),
               dict(B=1 << 16, Q=1 << 16), dict(max_hamming=-1), dict(max_hamming=37), dict(min_margin=-1.0), dict(min_margin=float("nan")),
               dict(min_margin=float("inf"))):
        assert decode(**kw) == T.ERR_ARG, kw
    for kw in (dict(width=4, height=4, pitch=4, frame_stride=16), dict(width=T.MAX_SIZE, height=T.MAX_SIZE, pitch=T.MAX_SIZE, frame_stride=T.MAX_SIZE ** 2),
               dict(B=1 << 10, Q=1 << 10), dict(B=1, frame_stride=0), dict(max_hamming=0), dict(max_hamming=36), dict(frame_stride=640 * 479 + 640)):
        assert decode(**kw) == T.ERR_FAMILY, kw


def test_missing_library_raises(monkeypatch):
    from accurate_aprilgroup_tracking_amd import tagcodelib
    monkeypatch.setattr(tagcodelib, "_lib", None)
    monkeypatch.setattr(tagcodelib, "LIB_PATH", "/nonexistent/libagt_tagcode.so")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tagcodelib.lib()


@pytest.mark.parametrize("name,frames", [("small", (0, 1)), ("dense", (0,)), ("c2", (0,))])
def test_numpy_statement_reads_the_rendered_truth(name, frames, cand):
    """every tag seen at under 60 degrees: no bit error, its own id, rot 0 -- with exact corners and with +-0.5 px of noise"""
    seq, codes = ts.sequence(name), ts.family_codes()
    for k in frames:
        front = ts.front_tags(seq, k)
        assert len(front) >= 8
        for noise in (0.0, 0.5):
            q = ts.quads(seq, k, noise)
            res = [tn.decode_quad(seq.frame(k), q[i], cand) for i in front]
            errs = sum(bin(r["word"] ^ int(codes[i])).count("1") for r, i in zip(res, front))
            low = min(r["margin"] for r in res)
            print("%s frame %d noise %.1f: %d tags, smallest edge %.1f px, %d bit errors, lowest margin %.2f" % (name, k, noise, len(front), ts.smallest_edge(q[front]), errs, low))
            assert errs == 0
            assert all(r["status"] == tn.OK and r["id"] == i and r["rot"] == 0 and r["hamming"] == 0 for r, i in zip(res, front))
            assert low > 2 * MARGIN_GATE
            if name == "c2":
                assert low == 97.5          # half of 225 - 30, reached exactly where a cell's sample sees one colour


@pytest.mark.parametrize("name", ["small", "dense", "c2"])
def test_numpy_statement_refuses_bare_background(name, cand):
    seq = ts.sequence(name)
    res = [tn.decode_quad(ts.bare_frame(seq), q, cand) for q in ts.background_quads(seq, 200)]
    print("%s: status counts %s, largest margin %.2f" % (name, np.bincount([r["status"] for r in res], minlength=7), max(r["margin"] for r in res)))
    assert all(r["status"] == tn.NO_MATCH or r["margin"] < MARGIN_GATE for r in res)
    assert not any(tn.decode_quad(ts.bare_frame(seq), q, cand, min_margin=MARGIN_GATE)["ok"] for q in ts.background_quads(seq, 200))


@pytest.mark.parametrize("name", ["small", "dense"])
def test_gpu_parity_inputs_stay_clear_of_the_threshold(name, cand):
    """the GPU parity tests compare a bit only where |I - thr| > 1e-6 and may leave out no tag quad and 2 % of the background quads:
    with the seeds used there the numpy statement alone leaves out none"""
    seq = ts.sequence(name)
    res = [tn.decode_quad(ts.bare_frame(seq), q, cand) for q in ts.background_quads(seq, 64)]
    for k in ((0, 1) if name == "small" else (0,)):
        for noise in (0.0, 0.5):
            res += [tn.decode_quad(seq.frame(k), q, cand) for q in ts.quads(seq, k, noise)]
    close = [r for r in res if r["d"] is not None and min(abs(v) for v in r["d"].values()) <= 1e-6]
    assert not close


def test_rolled_quads_give_the_rotation(cand):
    seq = ts.sequence("small")
    q = ts.quads(seq, 0)
    for i in ts.front_tags(seq, 0)[:4]:
        for k in range(4):
            r = tn.decode_quad(seq.frame(0), np.roll(q[i], -k, axis=0), cand, expected=int(i))
            assert (r["id"], r["rot"], r["hamming"], r["status"]) == (i, k, 0, tn.OK) and r["ok"] == int(k == 0)


def test_wrong_tag_and_covered_tag_fail_the_verdict(cand):
    seq = ts.sequence("c2")
    q, front = ts.quads(seq, 0), ts.front_tags(seq, 0)
    i, j = int(front[0]), int(front[1])
    assert tn.decode_quad(seq.frame(0), q[j], cand, expected=j)["ok"] == 1
    r = tn.decode_quad(seq.frame(0), q[j], cand, expected=i)
    assert r["status"] == tn.OK and r["id"] == j and r["ok"] == 0
    # the upper half of the tag (ring included) painted flat gray
    frame = seq.frame(0).copy()
    lo, hi = np.floor(q[i].min(axis=0)).astype(int) - 12, np.ceil(q[i].max(axis=0)).astype(int) + 12
    frame[max(lo[1], 0):int(round(q[i][:, 1].mean())), max(lo[0], 0):hi[0]] = 128
    assert tn.decode_quad(seq.frame(0), q[i], cand, expected=i)["ok"] == 1
    r = tn.decode_quad(frame, q[i], cand, expected=i)
    print("covered: status %d hamming %d margin %.2f" % (r["status"], r["hamming"], r["margin"]))
    assert r["ok"] == 0 and r["status"] in (tn.NO_MATCH, tn.INVERTED)


def test_tie_goes_to_the_lower_index_then_the_lower_rotation():
    codes = ts.family_codes()
    seq = ts.sequence("small")
    q, i = ts.quads(seq, 0), int(ts.front_tags(seq, 0)[0])
    dup = np.array([codes[40], codes[i], codes[41], codes[i]], np.uint64)
    r = tn.decode_quad(seq.frame(0), q[i], tn.candidates(dup))
    assert (r["id"], r["rot"], r["hamming"]) == (1, 0, 0)
    # a code equal to its own half turn matches at k = 0 and k = 2: the lower rotation wins
    sym = np.zeros((6, 6), np.uint8); sym[0, 1] = sym[5, 4] = sym[2, 3] = sym[3, 2] = 1
    assert np.array_equal(np.rot90(sym, 2), sym) and not np.array_equal(np.rot90(sym, 1), sym)
    word = tn.word_of(sym)
    hits = [(k, bin(word ^ cw).count("1")) for _, k, cw in tn.candidates([word])]
    assert [h for _, h in hits][0] == 0 and [h for _, h in hits][2] == 0


def test_degenerate_and_outside_quads_by_value(cand):
    seq = ts.sequence("small")
    frame = seq.frame(0)
    sq = np.array([[100.0, 100.0], [100.0, 140.0], [140.0, 140.0], [140.0, 100.0]], np.float32)
    for bad in (np.nan, np.inf, -np.inf, 1e30):
        for slot in range(8):
            q = sq.copy(); q.reshape(-1)[slot] = bad
            assert tn.decode_quad(frame, q, cand)["status"] == tn.DEGENERATE
    for q in (np.repeat(sq[:1], 4, axis=0), np.array([[0, 0], [10, 10], [20, 20], [30, 30]]), sq[[0, 2, 1, 3]], sq[[0, 1, 1, 3]]):
        assert tn.decode_quad(frame, q, cand)["status"] == tn.DEGENERATE
    assert tn.decode_quad(frame, sq, cand)["status"] in (tn.INVERTED, tn.NO_MATCH)
    assert tn.decode_quad(frame, sq[::-1], cand)["status"] in (tn.INVERTED, tn.NO_MATCH)          # the other orientation is a quad too


def test_family_generator_keeps_its_distance():
    codes = ts.family_codes()
    assert codes.dtype == np.uint64 and len(codes) == ts.N_CODES and len(set(codes.tolist())) == ts.N_CODES
    assert np.array_equal(codes, syn.make_tag_family(ts.N_CODES, ts.MIN_DISTANCE, 0))
    assert not np.array_equal(codes, syn.make_tag_family(ts.N_CODES, ts.MIN_DISTANCE, 1))
    rots = {(i, k): w for i, k, w in tn.candidates(codes)}
    worst = 36
    for (i, k), w in rots.items():
        for j in range(i, len(codes)):
            if j == i and k == 0:
                continue
            worst = min(worst, bin(w ^ int(codes[j])).count("1"))
    print("smallest distance over all pairs and rotations: %d" % worst)
    assert worst >= ts.MIN_DISTANCE
    bits = syn.family_bits(codes, [3, 5])
    assert bits.shape == (2, 6, 6) and tn.word_of(bits[0]) == int(codes[3]) and tn.word_of(bits[1]) == int(codes[5])
    with pytest.raises(ValueError):
        syn.make_tag_family(4, 30, 0, max_draws=2000)
    assert np.array_equal(syn.tag_bits(12, 1), np.random.default_rng(1 + 7919).integers(0, 2, size=(12, 6, 6)).astype(np.uint8))


def test_family_file_round_trip(tmp_path):
    from accurate_aprilgroup_tracking_amd import formats, tag_decode
    codes = ts.family_codes()
    formats.save_tag_family(tmp_path / "family.npz", codes, name="synthetic36")
    fam = formats.load_tag_family(tmp_path / "family.npz")
    assert isinstance(fam, tag_decode.TagFamily) and fam.name == "synthetic36" and fam.bits_per_side == 6
    assert fam.codes.dtype == np.uint64 and np.array_equal(fam.codes, codes) and len(fam) == len(codes)
    assert np.array_equal(fam.bits([2]), syn.family_bits(fam, [2]))
    np.savez(tmp_path / "short.npz", codes=codes)
    with pytest.raises(ValueError, match="bits_per_side"):
        formats.load_tag_family(tmp_path / "short.npz")
    with pytest.raises(ValueError):
        tag_decode.TagFamily(np.array([1 << 36], np.uint64))
    with pytest.raises(ValueError):
        tag_decode.TagFamily(codes, bits_per_side=5)


def test_records_to_detections_undoes_the_rotation(cand):
    from accurate_aprilgroup_tracking_amd import tag_decode
    seq = ts.sequence("c2")
    q, i = ts.quads(seq, 0), int(ts.front_tags(seq, 0)[0])
    rolled = np.roll(q[i], -3, axis=0)
    res = [tn.decode_quad(seq.frame(0), rolled, cand), tn.decode_quad(ts.bare_frame(seq), rolled, cand)]
    rec = np.zeros(2, tn.RECORD_DTYPE)
    for k, r in enumerate(res):
        for f in tn.RECORD_DTYPE.names:
            rec[k][f] = r[f]
    dets = tag_decode.records_to_detections(rec, [rolled, rolled], [r["H"] for r in res], "synthetic36")
    assert len(dets) == 1
    d = dets[0]
    assert (d.tag_id, d.hamming, d.tag_family, d.decision_margin) == (i, 0, b"synthetic36", res[0]["margin"])
    assert np.array_equal(d.corners, q[i].astype(np.float64))
    proj = np.c_[tn.SQUARE, np.ones(4)] @ d.homography.T
    assert np.abs(proj[:, :2] / proj[:, 2:] - d.corners).max() < 1e-9 and d.homography[2, 2] == 1.0
    assert np.abs(d.center - d.homography[:2, 2]).max() == 0.0
