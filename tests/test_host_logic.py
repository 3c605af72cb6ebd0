"""CPU-only: the host side above the C-ABI (halo2 mirror constants, shard arithmetic) against the fixtures and the oracle."""
import numpy as np
import pytest

import __graft_entry__ as ge
from oracle import cref, pyref


@pytest.fixture(scope="module")
def zk():
    return ge.load_package()


@pytest.mark.parametrize("which,k", [("chunk_protocol", 25), ("batch_proof", 26)])
def test_evaluation_domain_constants_match_reference_fixtures(zk, kat, which, k):
    """EvaluationDomain::new derives omega from ROOT_OF_UNITY; the released protocol files store the same value (KAT A1/A2)."""
    pr = kat[which] if which == "chunk_protocol" else kat[which]["protocol"]
    dom = zk.halo2.EvaluationDomain(2, k)
    assert dom.omega.tolist() == pr["domain"]["gen"]
    assert dom.omega_inv.tolist() == pr["domain"]["gen_inv"]
    assert dom.ifft_divisor.tolist() == pr["domain"]["n_inv"]


def test_extended_domain_rule(zk):
    h2 = zk.halo2
    for j, k, want in [(2, 10, 10), (3, 10, 11), (4, 10, 12), (5, 10, 12), (6, 10, 13), (5, 26, 28)]:
        dom = h2.EvaluationDomain(j, k)
        assert dom.extended_k == want
        assert pow(dom._extended_omega, 1 << dom.extended_k, h2.R_MOD) == 1 and pow(dom._extended_omega, 1 << (dom.extended_k - 1), h2.R_MOD) != 1
        assert pow(dom._extended_omega, 1 << (dom.extended_k - k), h2.R_MOD) == dom._omega
    with pytest.raises(AssertionError):
        h2.EvaluationDomain(9, 26)      # would need 2^29 > two-adicity 28
    assert (h2.fr(h2.FR_ZETA) == cref.fr_mont(pyref.FR_ZETA)).all()
    for v in (0, 1, 7, h2.R_MOD - 1, 1 << 200):
        assert (h2.fr(v) == cref.fr_mont(v)).all() and h2.fr_to_int(h2.fr(v)) == v % h2.R_MOD


def test_shard_ranges(zk):
    sr = zk.distributed.shard_range
    for n in (0, 1, 7, 8, 1000, 1 << 26):
        for world in (1, 2, 3, 4, 8):
            cover = []
            for r in range(world):
                lo, hi = sr(n, r, world)
                assert 0 <= lo <= hi <= n
                cover.append((lo, hi))
            assert cover[0][0] == 0 and cover[-1][1] == n
            assert all(cover[i][1] == cover[i + 1][0] for i in range(world - 1))
            sizes = [hi - lo for lo, hi in cover]
            assert max(sizes) - min(sizes) <= 1


def test_params_file_format_roundtrip(zk, tmp_path):
    """SerdeFormat::RawBytes layout of params{k} and the exact-length rule of prover::load_params."""
    h2 = zk.halo2
    assert h2.params_file_size(26) == 8589934852 and h2.params_file_size(20) == 134217988   # the sizes behind [REF params-sha256sum:1-5]
    k = 3
    g, gl, _, _ = cref.srs_setup(k, cref.fr_mont(0xABCDEF), cref.fr_mont(pyref.omega(k)))
    path = str(tmp_path / "params3")
    g2, s_g2 = bytes(range(128)), bytes(range(128, 256))
    h2.write_params(path, k, g, gl, g2, s_g2)
    k2, a, b, c, d = h2.read_params(path)
    assert k2 == k and (a == g).all() and (b == gl).all() and c == g2 and d == s_g2
    with open(path, "ab") as f:
        f.write(b"\\0")
    with pytest.raises(ValueError):
        h2.read_params(path)


@pytest.mark.parametrize("vk,proto,npts", [("vk_chunk", "chunk_protocol", 7), ("vk_batch_agg", "batch_proof", 9)])
def test_g1_wire_codec_against_released_vkeys(zk, kat, vk, proto, npts):
    """the host mirror's compressed-point codec on the reference's own .vkey bytes and protocol points (KAT A4), and on proof words (A5/A6)."""
    h2 = zk.halo2
    raw = bytes.fromhex(kat[vk])
    pr = kat[proto] if proto == "chunk_protocol" else kat[proto]["protocol"]
    for i in range(npts):
        word = raw[8 + 32 * i: 40 + 32 * i]
        pt = np.array(pr["preprocessed"][i]["x"] + pr["preprocessed"][i]["y"], dtype=np.uint64)
        assert (h2.g1_from_bytes(word) == pt).all() and h2.g1_to_bytes(pt) == word
        assert (h2.g1_from_bytes(word) == cref.g1_decompress(word)).all()
    proof = bytes.fromhex(kat["chunk_proof"]["proof"])
    for i in list(range(9)) + [26, 27]:
        w = proof[32 * i: 32 * i + 32]
        assert h2.g1_to_bytes(h2.g1_from_bytes(w)) == w and cref.g1_is_on_curve(h2.g1_from_bytes(w))
    assert h2.g1_to_bytes(np.zeros(12, dtype=np.uint64)) == bytes(32) and (h2.g1_from_bytes(bytes(32)) == 0).all()
    with pytest.raises(ValueError):
        h2.g1_from_bytes((4).to_bytes(32, "little"))      # x = 4: 4^3 + 3 = 67 is not a square mod p


def test_signed_digit_recoding_algorithm():
    """The recoding k_msm_digits applies (restated here in integers): take the smaller of k and r - k, cut it into c-bit windows from
    the bottom, turn raw values above 2^(c-1) into negative digits with a carry.  Properties the kernels rely on: W = ceil(255 / c)
    windows always absorb the last carry, |digit| <= 2^(c-1) (bucket index = |digit| - 1 < 2^(c-1)), and the digits reconstruct
    +-k (mod r) with the sign that moved to the point."""
    import random
    R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
    rng = random.Random(2024)

    def recode(k, c):
        flip = (R - k) < k
        v = R - k if flip else k
        W = (255 + c - 1) // c
        half, digits, carry = 1 << (c - 1), [], 0
        for w in range(W):
            raw = ((v >> (w * c)) & ((1 << c) - 1)) + carry
            if raw > half:
                d, carry = raw - (1 << c), 1
            else:
                d, carry = raw, 0
            digits.append(-d if flip else d)
        return digits, carry

    samples = [0, 1, 2, R - 1, R - 2, (R - 1) // 2, (R + 1) // 2, (1 << 253) - 1, (1 << 252), R >> 1, 0x1234567890abcdef1234567890abcdef1234567890abcdef]
    samples += [rng.randrange(R) for _ in range(300)] + [rng.randrange(1 << 64) for _ in range(50)] + [R - rng.randrange(1 << 64) for _ in range(50)]
    for c in range(2, 25):
        for k in samples:
            digits, carry = recode(k, c)
            assert carry == 0, (c, hex(k))
            assert all(abs(d) <= 1 << (c - 1) for d in digits)
            assert sum(d << (w * c) for w, d in enumerate(digits)) % R == k % R, (c, hex(k))
        # small negative values use ONE window once c covers them
        if c >= 8:
            digits, _ = recode(R - 100, c)
            assert digits[0] == -100 and all(d == 0 for d in digits[1:])


def test_accumulate_segment_rule_covers_every_entry():
    """msm_seg_eff (msm.hpp), restated in integers: the accumulate launch is sized for the worst case (threads = ceil(emax / seg_max) rounded to
    workgroups), and every kernel derives the segment from the actual entry count as clamp(ceil(total / (fill % of the threads)), seg_min,
    seg_max).  Whatever the count, threads * segment must cover it, and a full column must get the worst-case segment back."""
    import random

    def seg_eff(total, threads, seg_max, seg_min, fill_pct):
        target = (threads * min(fill_pct, 100) + 99) // 100          # the kernel clamps the percentage: more than the launched threads cannot take entries
        sg = (total + target - 1) // max(target, 1)
        return min(max(sg, seg_min), seg_max)

    rng = random.Random(7)
    for _ in range(20000):
        emax = rng.choice([rng.randrange(1, 1 << 12), rng.randrange(1, 1 << 24), rng.randrange(1, (1 << 32) - 1)])
        want_threads = 256 * 256 * 16
        seg_max = min(max((emax + want_threads - 1) // want_threads, 16), 4096)
        threads = -(-(-(-emax // seg_max)) // 256) * 256
        seg_min = min(rng.choice([1, 16, 64, 256, 4096]), seg_max)
        fill = rng.choice([2, 20, 40, 60, 100, 126])
        total = rng.choice([0, 1, emax, emax // 7, rng.randrange(0, emax + 1)])
        sg = seg_eff(total, threads, seg_max, seg_min, fill)
        assert seg_min <= sg <= seg_max
        assert threads * sg >= total, (emax, total, threads, sg)
        if total == emax and fill <= 100:
            assert sg == seg_max or sg * threads >= emax      # nothing is lost for a column in which every digit is non-zero


def test_build_is_content_hashed_per_translation_unit():
    """scroll-prover_amd/build.py decides staleness by content (sha256 of every file a unit includes + the flags), so a copied tree -- the GPU
    box's snapshot -- never rebuilds what was built here, and a header change rebuilds exactly the units that include it."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("_b", os.path.join(root, "scroll-prover_amd", "build.py"))
    b = importlib.util.module_from_spec(spec); spec.loader.exec_module(b)
    b.build()
    assert not b.needs_build()
    assert b.needs_build(extra_flags=["-DSOMETHING=1"])                       # other flags = another build
    h = {u: b._unit_hash(u, []) for u in b.UNITS}
    assert len(set(h.values())) == len(b.UNITS)
    closure = {}
    b._closure(os.path.join(b.CSRC, "lib_core.hip"), closure)
    names = {os.path.basename(p) for p in closure}
    assert "lib_common.hpp" in names and "mi355zk.h" in names and "msm.hpp" not in names and "ntt29.hpp" not in names   # lib_core launches no kernel
    closure = {}
    b._closure(os.path.join(b.CSRC, "lib_ntt.hip"), closure)
    assert "ntt29.hpp" in {os.path.basename(p) for p in closure} and "msm.hpp" not in {os.path.basename(p) for p in closure}


def test_host_compact_nonzero_needs_no_device():
    """the host half of the sparse upload (include/mi355zk.h mi355_host_compact_nonzero): indices and values of the non-zero cells in order, any thread count, ragged sizes"""
    import numpy as np
    import __graft_entry__ as ge
    h2 = ge.load_package().halo2
    rng = np.random.default_rng(5)
    for n in (0, 1, 1000, (1 << 17) + 13):
        col = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
        col[rng.random(n) < 0.7] = 0
        want = np.nonzero(col.any(axis=1))[0].astype(np.uint32)
        for threads in (1, 3, 16):
            idx, vals = h2.compact_nonzero(col, threads)
            assert (idx == want).all() and (vals == col[want]).all()


def test_full_range_operand_generators():
    """tests/gpu_common.py: the adversarial word pool is a duplicate-free set of legal words, and every rand_fr_full draw of the full-range GPU tests
    has at least 60 % of its words at or above 2^252 (expected 1 - 2^252 / r = 66.9 %, standard deviation 1.5 % at n = 1000), where rand_fr has none."""
    from tests import gpu_common as gc
    R = pyref.R_MOD
    ints = gc.adversarial_fr_ints()
    words = gc.adversarial_fr_words()
    assert all(0 <= v < R for v in ints) and len(set(ints)) == len(ints) >= 50
    assert words.shape == (len(ints), 4) and words.dtype == np.uint64 and gc.words_to_ints(words) == ints and gc.below_r(words).all()
    mont = (1 << 256) % R
    for v in [0, 1, 2, R - 1, R - 2, (R - 1) // 2, (R + 1) // 2, mont, R - mont, 2 * mont % R, gc.ALL_ONES_LIMBS, (1 << 252) - 1, 1 << 252, 1 << 253,
              int("55" * 32, 16) % R, int("AA" * 32, 16) % R] + [(1 << (29 * i)) + d for i in range(1, 9) for d in (-1, 0, 1)] + [(1 << (32 * i)) - d for i in range(1, 8) for d in (1, 0)]:
        assert v in ints, hex(v)
    assert gc.ALL_ONES_LIMBS < R and all((gc.ALL_ONES_LIMBS >> (29 * i)) & 0x1FFFFFFF == 0x1FFFFFFF for i in range(8)) and gc.ALL_ONES_LIMBS + (1 << 232) >= R
    a, b = gc.pool_pairs(words)
    m = len(ints)
    assert a.shape == b.shape == (m * m, 4) and set(zip(gc.words_to_ints(a), gc.words_to_ints(b))) == {(x, y) for x in ints for y in ints}
    assert (gc.tile_words(words, 2 * m + 3)[m:2 * m] == words).all()
    r0 = gc.rand_fr(np.random.default_rng(1), 1000, full=False)
    assert (r0[:, 3] < np.uint64(1 << 60)).all()                       # what the older generator covers
    for name, (seed, sizes) in gc.FULL_RANGE_DRAWS.items():
        big = gc.full_range(name, max(sizes))
        assert big.shape == (max(sizes), 4) and big.dtype == r0.dtype and gc.below_r(big).all()
        for n in sizes:
            if n >= 1000:
                share = float((big[:n, 3] >= np.uint64(1 << 60)).mean())
                assert share >= 0.60, (name, seed, n, share)
        assert (gc.full_range(name, 1000) == big[:1000]).all()        # a shorter draw is a prefix


def test_scan_oracle_agrees_with_integers_on_the_pool():
    """the C oracle's batch_invert / prefix_sum / prefix_product on the adversarial word pool against Python integers: what the full-range GPU scan
    tests lean on"""
    from tests import gpu_common as gc
    R = pyref.R_MOD
    rinv, mont = pow(1 << 256, -1, R), (1 << 256) % R
    ints, pool = gc.adversarial_fr_ints(), gc.adversarial_fr_words()
    assert gc.words_to_ints(cref.batch_invert(pool)) == [pow(v * rinv, -1, R) * (1 << 256) % R if v else 0 for v in ints]
    z, t = cref.prefix_sum(pool)
    acc, want = 0, []
    for v in ints:
        want.append(acc); acc = (acc + v) % R
    assert gc.words_to_ints(z) == want and gc.words_to_ints(t)[0] == acc
    z, t = cref.prefix_product(pool[1:])
    acc, want = mont, []
    for v in ints[1:]:
        want.append(acc); acc = acc * v * rinv % R
    assert gc.words_to_ints(z) == want and gc.words_to_ints(t)[0] == acc


def test_adversarial_curve_point_pools():
    """tests/gpu_common.py: every point of the adversarial G1 / G2 pools is on its curve, none is listed twice, none has the x word 0 (the device's
    identity test reads x alone), every pool word lifted to a coordinate within LIFT_MAX = 8, and every y-triple (x, beta x, beta^2 x) sums to the identity.
    Observed: 54 words; "mont": 189 G1 points (34 triples), x lifts within 3 (32 words at 0), y within 3 (12 at 0), 284 twist points within 4;
    "canonical": 182 G1 points (34 triples), x within 3 (25 at 0), y within 4 (10 at 0), 288 twist points within 5."""
    from tests import gpu_common as gc
    P = pyref.P_MOD
    ints = gc.adversarial_fq_ints()
    assert len(set(ints)) == len(ints) >= 50 and all(0 <= v < P for v in ints)
    mont = (1 << 256) % P
    for v in [0, 1, 2, P - 1, P - 2, (P - 1) // 2, (P + 1) // 2, mont, P - mont, 2 * mont % P, gc.ALL_ONES_LIMBS, (1 << 252) - 1, 1 << 252, 1 << 253,
              int("55" * 32, 16) % P, int("AA" * 32, 16) % P] + [(1 << (29 * i)) + d for i in range(1, 9) for d in (-1, 0, 1)] + [(1 << (32 * i)) - d for i in range(1, 8) for d in (1, 0)]:
        assert v in ints, hex(v)
    assert pow(gc.FQ_BETA, 3, P) == 1 and gc.FQ_BETA != 1 and gc.LIFT_MAX == 8
    rinv = pow(1 << 256, -1, P)
    for reading in ("mont", "canonical"):
        pts, words, dist = gc.adversarial_g1_points(reading)
        py, kind, triples = gc.adversarial_g1_info(reading)
        m = pts.shape[0]
        assert pts.shape == (m, 8) and pts.dtype == np.uint64 and words.shape == (m, 4) and dist.shape == (m,) and m >= 150
        assert len({p.tobytes() for p in pts}) == m and len(set(py)) == m
        assert int(np.abs(dist).max()) <= 8
        assert pts[:, :4].any(axis=1).all(), "no point has the x word 0"
        for i in range(m):
            assert pyref.g1_is_on_curve(py[i]) and cref.g1_is_on_curve(pts[i])
            assert pyref.g1_affine_from_limbs(pts[i, :4], pts[i, 4:]) == py[i]
            coord = gc.words_to_ints(pts[i:i + 1, :4] if kind[i] == "x" else pts[i:i + 1, 4:])[0]      # the ABI word of the lifted coordinate
            if reading == "canonical":
                coord = coord * rinv % P
            assert coord == gc.words_to_ints(words[i:i + 1])[0] + int(dist[i]), "the word the point was built for, at its distance"
        for fam in "xy":                                                  # every pool word has a point of either family within reach (a point two words share is listed once)
            have = [gc.words_to_ints(words[i:i + 1])[0] + int(dist[i]) for i in range(m) if kind[i] == fam]
            assert all(min(abs(w - h) for h in have) <= 8 for w in ints), fam
        assert len(triples) >= 30 and {i for t in triples for i in t} >= {i for i in range(m) if kind[i] == "y"}      # a member may have been listed as an x lift before
        for t in triples:
            a, b, c = (py[i] for i in t)
            assert a[1] == b[1] == c[1] and len({a[0], b[0], c[0]}) == 3
            assert pyref.g1_add(pyref.g1_add(a, b), c) is None
            acc = np.zeros(12, dtype=np.uint64)
            for i in t:
                acc = cref.g1_add_affine(acc, pts[i])
            assert not acc[8:].any(), "and the C oracle says so too"
        for p, q in zip(gc.g1_neg_words(pts), py):
            assert pyref.g1_affine_from_limbs(p[:4], p[4:]) == pyref.g1_neg(q)
        non = gc.adversarial_fq_non_lifting(reading)
        val = (lambda w: w * rinv % P) if reading == "mont" else (lambda w: w)
        assert 0 in non and all(gc.fq_sqrt((val(w) ** 3 + 3) % P) is None or val(w) == 0 for w in non) and len(non) >= 10
        g2, g2py, g2d = gc.adversarial_g2_points(reading)
        assert g2.shape == (len(g2py), 16) and len(set(g2py)) == len(g2py) >= 250 and int(np.abs(g2d).max()) <= 8
        for q, w in zip(g2py, g2):
            assert pyref.g2_is_on_curve(q) and cref.g2_is_on_curve(w) and list(w) == pyref.g2_to_limbs(q)
        assert any(q[0][1] == 0 for q in g2py) and any(q[0][0] < 8 and q[0][1] for q in g2py) if reading == "canonical" else True
    assert not cref.g2_in_subgroup(gc.adversarial_g2_points()[0][0]), "twist points outside the subgroup of order r"


def test_oracles_agree_on_the_adversarial_points():
    """what the GPU tests lean on: the C oracle against Python integers ON these points -- an MSM over the G1 pool, and cref.g2_mul on twist points
    outside the order-r subgroup (the scalar acts as an integer there)"""
    from tests import gpu_common as gc
    P, R = pyref.P_MOD, pyref.R_MOD
    pts, _, _ = gc.adversarial_g1_points("mont")
    py, _, _ = gc.adversarial_g1_info("mont")
    sc = gc.full_range("msm", pts.shape[0])
    can = gc.words_to_ints(cref.f_to_canonical_vec(cref.FR, sc))
    for lo in (0, pts.shape[0] - 48):
        want = pyref.msm(can[lo:lo + 48], py[lo:lo + 48])
        got = cref.g1_to_affine(cref.best_multiexp(sc[lo:lo + 48], pts[lo:lo + 48]))
        assert pyref.g1_affine_from_limbs(got[:4], got[4:]) == want
    g2, g2py, _ = gc.adversarial_g2_points()
    rinv = pow(1 << 256, -1, P)
    for i in range(0, len(g2py), 9):
        k = (R - 1, pyref.FR_ZETA, can[i % len(can)])[i % 3]
        got = cref.g2_mul(g2[i], cref.fr_mont(k))
        assert list(got) == pyref.g2_to_limbs(pyref.g2_mul(g2py[i], k)), i
