"""-m gpu: the compressed-point codec of G1 on the device (mi355_g1_decompress_* / mi355_g1_compress_*, csrc/g1codec.hpp) against cref word for word, its error
reporting (the smallest rejected index at any grid size), the SerdeFormat::Processed route of mi355_srs_load_params_file against the RawBytes route, the
sharded load over two device slots, the codec at 2^24 (and 2^26 where memory allows) and the compiled caller tests/cpp/test_g1_codec."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge
from oracle import cref, pyref
from tests.gpu_common import affine_of, rand_fr

pytestmark = pytest.mark.gpu
TAU = 0x5343524F4C4C0C0D
P = pyref.P_MOD
SIZES = [1, 2, 63, 64, 65, 1000, 1 << 16, (1 << 18) + 3]
NONE = (1 << 64) - 1


@pytest.fixture(scope="module")
def zk():
    pkg = ge.load_package()
    pkg.init(0)
    return pkg


def word_of(x: int, sign: int = 0) -> bytes:
    return (x | (sign << 254)).to_bytes(32, "little")


def non_residue_words(count):
    out, x = [], 1
    while len(out) < count:
        x += 1
        rhs = (x * x * x + 3) % P
        if pow(rhs, (P - 1) // 2, P) == P - 1:
            out.append(word_of(x, len(out) & 1))
    return out


@pytest.fixture(scope="module")
def pool(zk):
    """2^18 + 3 points that look random (the Lagrange basis of a synthetic SRS), identities sprinkled in, with cref's words for them"""
    h2 = zk.halo2
    params = h2.ParamsKZG.setup(19, TAU)
    n = SIZES[-1]
    pts = params.read_g(lagrange=True)[:n].copy()
    params.release()
    rng = np.random.default_rng(77)
    for i in [0, 5, 64, 999, 65535, n - 1] + list(rng.integers(0, n, size=40)):
        pts[int(i)] = 0
    words = np.frombuffer(b"".join(cref.g1_compress(p) for p in pts), dtype=np.uint8).reshape(n, 32).copy()
    signs = (words[:, 31] >> 6) & 1
    assert 0.4 < signs.mean() < 0.6, "both parities occur"
    return pts, words


@pytest.mark.parametrize("n", SIZES)
def test_codec_equals_cref_word_for_word(zk, pool, n):
    h2 = zk.halo2
    pts, words = pool[0][:n], pool[1][:n]
    want = np.stack([cref.g1_decompress(w.tobytes()) for w in words])      # the oracle's decompression, not the points the words came from
    assert (want == pts).all()
    got = h2.g1_decompress(words)                                            # host pointers
    assert got.shape == (n, 8) and (got == want).all()
    assert (h2.g1_compress(pts) == words).all()
    dw = torch.from_numpy(words.reshape(-1)).cuda()                          # device pointers
    dp = h2.g1_decompress(dw)
    assert (dp.cpu().numpy().view(np.uint64).reshape(n, 8) == want).all()
    dc = h2.g1_compress(dp)
    torch.cuda.synchronize()
    assert torch.equal(dc, dw), "compress(decompress(w)) == w"
    assert torch.equal(h2.g1_decompress(h2.g1_compress(torch.from_numpy(pts.reshape(-1)).cuda())), dp), "decompress(compress(P)) == P"


@pytest.mark.parametrize("blocks", ["", "1", "333"])
def test_rejected_words_report_the_smallest_index(zk, pool, blocks):
    h2, capi = zk.halo2, zk._capi
    lib, ptr = capi.lib(), capi.ptr
    n = 50000
    words = pool[1][:n].copy()
    rng = np.random.default_rng(91)
    bad_words = non_residue_words(5) + [word_of(P), word_of(P + 1, 1), word_of((1 << 254) - 1), word_of(0, 1)]
    for w in bad_words:                                                      # every rejected class decodes as the oracle says
        assert cref.g1_decompress(w) is None
    idx = rng.permutation(np.arange(1000, n))[:len(bad_words)]               # planted in random order at known indices
    for i, w in zip(idx, bad_words):
        words[int(i)] = np.frombuffer(w, dtype=np.uint8)
    os.environ.pop("MI355_G1_CODEC_BLOCKS", None)
    if blocks:
        os.environ["MI355_G1_CODEC_BLOCKS"] = blocks
    try:
        out = np.full((n, 8), 0xAB, dtype=np.uint64); bad = C.c_uint64(0)
        assert lib.mi355_g1_decompress_host(ptr(words), ptr(out), n, C.byref(bad)) == capi.EBADARG
        assert bad.value == int(idx.min()) and str(int(idx.min())) in lib.mi355_last_error().decode()
        for i in idx:
            assert not out[int(i)].any(), "a rejected slot holds the identity"
        ok = np.ones(n, dtype=bool); ok[idx] = False
        assert (out[ok] == pool[0][:n][ok]).all(), "the other slots are decoded all the same"
        dw = torch.from_numpy(words.reshape(-1)).cuda(); dout = torch.empty(n * 64, dtype=torch.uint8, device="cuda"); bad = C.c_uint64(0)
        assert lib.mi355_g1_decompress_dev(ptr(dw), ptr(dout), n, C.byref(bad)) == capi.EBADARG and bad.value == int(idx.min())
        with pytest.raises(zk.Mi355Error) as e:
            h2.g1_decompress(words)
        assert e.value.code == capi.EBADARG and e.value.index == int(idx.min())
        # one planted word: that index, whichever class
        for w in (bad_words[0], bad_words[5], bad_words[-1]):
            one = pool[1][:n].copy(); one[n - 1] = np.frombuffer(w, dtype=np.uint8)
            assert lib.mi355_g1_decompress_host(ptr(one), ptr(out), n, C.byref(bad)) == capi.EBADARG and bad.value == n - 1
    finally:
        os.environ.pop("MI355_G1_CODEC_BLOCKS", None)


def test_argument_checks(zk, pool):
    capi = zk._capi
    lib, ptr = capi.lib(), capi.ptr
    out = np.full((4, 8), 0xCD, dtype=np.uint64); words = pool[1][:4].copy(); bad = C.c_uint64(5)
    assert lib.mi355_g1_decompress_host(ptr(words), ptr(out), 0, C.byref(bad)) == capi.OK and bad.value == NONE
    assert (out == 0xCD).all(), "n = 0 writes nothing"
    assert lib.mi355_g1_compress_host(ptr(out), ptr(words), 0) == capi.OK and (words == pool[1][:4]).all()
    assert lib.mi355_g1_decompress_dev(None, None, 0, None) == capi.OK and lib.mi355_g1_compress_dev(None, None, 0) == capi.OK
    assert lib.mi355_g1_decompress_host(None, ptr(out), 4, None) == capi.EBADARG
    assert lib.mi355_g1_decompress_host(ptr(words), None, 4, None) == capi.EBADARG
    assert lib.mi355_g1_compress_host(None, ptr(words), 4) == capi.EBADARG and lib.mi355_g1_compress_host(ptr(out), None, 4) == capi.EBADARG
    d = torch.zeros(4 * 96, dtype=torch.uint8, device="cuda")
    assert lib.mi355_g1_decompress_dev(None, ptr(d), 4, None) == capi.EBADARG and lib.mi355_g1_compress_dev(ptr(d), None, 4) == capi.EBADARG
    assert lib.mi355_g1_decompress_dev(C.c_void_p(d.data_ptr()), C.c_void_p(d.data_ptr() + 64), 4, None) == capi.EBADARG   # overlap
    assert lib.mi355_g1_decompress_host(ptr(words), ptr(out), 4, None) == capi.OK                                            # first_bad_out is optional
    assert (out == pool[0][:4]).all()


def test_profile_names(zk, pool):
    capi = zk._capi
    lib = capi.lib()
    capi.check(lib.mi355_profile_enable(1)); capi.check(lib.mi355_profile_reset())
    try:
        zk.halo2.g1_compress(zk.halo2.g1_decompress(pool[1][:4096]))
        for name in (b"g1_decompress", b"g1_compress"):
            ms, launches = C.c_double(), C.c_uint64()
            capi.check(lib.mi355_profile_get(name, C.byref(ms), C.byref(launches)))
            assert launches.value == 1 and ms.value > 0, name
    finally:
        capi.check(lib.mi355_profile_enable(0))


# ---- the Processed params loader
def commit_of(params, scal):
    return affine_of(params.commit_lagrange(scal))


@pytest.mark.parametrize("k", [10, 16, 20])
def test_processed_file_loads_to_the_same_bases_as_rawbytes(zk, tmp_path, k):
    h2 = zk.halo2
    n = 1 << k
    src = h2.ParamsKZG.setup(k, TAU + k)
    raw, proc = str(tmp_path / "raw"), str(tmp_path / "proc")
    src.write(raw); src.write(proc, format="processed")
    assert os.path.getsize(raw) == h2.params_file_size(k) and os.path.getsize(proc) == h2.params_file_size(k, "processed")
    a, b = h2.params_from_file(raw, validate=True), h2.params_from_file(proc, format="processed")
    try:
        assert b.k == k
        for lag in (False, True):
            pa, pb = a.read_g(lagrange=lag), b.read_g(lagrange=lag)
            assert pa.tobytes() == pb.tobytes() and pa.tobytes() == src.read_g(lagrange=lag).tobytes()
        assert b.g2 == src.g2 and b.s_g2 == src.s_g2 and a.g2 == b.g2 and a.s_g2 == b.s_g2 and any(b.s_g2)
        scal = rand_fr(np.random.default_rng(k), n)
        assert (commit_of(a, scal) == commit_of(b, scal)).all() and (affine_of(a.commit(scal)) == affine_of(b.commit(scal))).all()
        if k == 10:   # the file itself, against a writer that knows only the oracle
            g, gl = src.read_g(), src.read_g(lagrange=True)
            want = (k).to_bytes(4, "little") + b"".join(cref.g1_compress(p) for p in g) + b"".join(cref.g1_compress(p) for p in gl)
            body = open(proc, "rb").read()
            assert body[:len(want)] == want and body[len(want):] == h2.g2_to_bytes(src.g2) + h2.g2_to_bytes(src.s_g2)
    finally:
        for p in (a, b, src):
            p.release()


def handle_probe(zk):
    """registers and releases a one-point basis: handles are handed out in sequence, so two probes tell how many were registered in between"""
    capi = zk._capi
    h = C.c_uint64()
    capi.check(capi.lib().mi355_srs_register_host(capi.ptr(np.zeros((1, 8), dtype=np.uint64)), 1, C.byref(h)))
    capi.check(capi.lib().mi355_srs_release(h.value))
    return h.value


def test_processed_loader_rejections(zk, tmp_path):
    h2, capi = zk.halo2, zk._capi
    k = 12
    n = 1 << k
    src = h2.ParamsKZG.setup(k, TAU + 1)
    raw, proc = str(tmp_path / "raw"), str(tmp_path / "proc")
    src.write(raw); src.write(proc, format="processed")
    src.release()
    body = bytearray(open(proc, "rb").read())

    def load(path, **kw):
        before = handle_probe(zk)
        with pytest.raises(zk.Mi355Error) as e:
            h2.params_from_file(path, **kw)
        assert e.value.code == capi.EBADARG
        assert handle_probe(zk) == before + 1, "a failed load registers nothing"
        return str(e.value)

    # one byte corrupted into a non-residue, in each basis
    for basis, base in (("g", 4), ("g_lagrange", 4 + 32 * n)):
        idx = 1234
        off = base + 32 * idx
        bad = bytearray(body)
        for delta in range(1, 256):
            bad[off] = (body[off] + delta) & 0xFF
            if cref.g1_decompress(bytes(bad[off:off + 32])) is None:
                break
        else:
            pytest.fail("no single-byte change made a non-residue")
        p = str(tmp_path / ("bad_" + basis)); open(p, "wb").write(bad)
        msg = load(p, format="processed")
        assert f"{basis}[{idx}]" in msg, msg
    # a corrupted G2 word (x off the twist) is refused too
    bad = bytearray(body); off = len(body) - 64
    for delta in range(1, 256):
        bad[off] = (body[off] + delta) & 0xFF
        p = str(tmp_path / "bad_g2"); open(p, "wb").write(bad)
        try:
            h2.params_from_file(p, format="processed").release()
        except zk.Mi355Error as e:
            assert e.code == capi.EBADARG and "s_g2" in str(e)
            break
    else:
        pytest.fail("every single-byte change of s_g2's x decoded")
    # truncated; Processed without bit 1 (the parent's message, byte for byte); RawBytes with bit 1
    p = str(tmp_path / "short"); open(p, "wb").write(body[:-1])
    assert "file length" in load(p, format="processed")
    msg = load(proc)
    assert msg.endswith("srs_load_params_file: file length does not match 4 + 2 * 2^k * 64 + 256 (load_params rejects it too)"), msg
    assert "4 + 2 * 2^k * 32 + 128" in load(raw, format="processed")


def test_sharded_processed_load_over_two_device_slots(tmp_path):
    pkg = ge.load_package()
    pkg.init(0)
    h2 = pkg.halo2
    k = 12
    src = h2.ParamsKZG.setup(k, TAU + 2)
    proc = str(tmp_path / "proc"); src.write(proc, format="processed")
    g, gl, g2, s_g2 = src.read_g(), src.read_g(lagrange=True), src.g2, src.s_g2
    src.release()
    pkg.shutdown()
    os.environ.update({"MI355_ALLOW_DUP_DEVICES": "1", "MI355_SHARD_MIN_LOG": "8"})
    try:
        pkg.init([0, 0])
        b = h2.params_from_file(proc, format="processed")
        assert b.read_g().tobytes() == g.tobytes() and b.read_g(lagrange=True).tobytes() == gl.tobytes() and (b.g2, b.s_g2) == (g2, s_g2)
        scal = rand_fr(np.random.default_rng(3), 1 << k)
        got = commit_of(b, scal)
        again = str(tmp_path / "again"); b.write(again, format="processed")          # the writer's route for a sharded basis
        assert open(again, "rb").read() == open(proc, "rb").read()
        bad = bytearray(open(proc, "rb").read()); idx = (1 << k) - 7                  # a rejected word in the second shard: the index is the basis's, not the shard's
        bad[4 + 32 * idx: 4 + 32 * idx + 32] = non_residue_words(1)[0]
        open(again, "wb").write(bad)
        with pytest.raises(pkg.Mi355Error) as e:
            h2.params_from_file(again, format="processed")
        assert f"g[{idx}]" in str(e.value)
        b.release()
    finally:
        pkg.shutdown()
        for v in ("MI355_ALLOW_DUP_DEVICES", "MI355_SHARD_MIN_LOG"):
            os.environ.pop(v, None)
        pkg.init(0)
    a = h2.params_from_file(proc, format="processed")
    assert (commit_of(a, scal) == got).all()
    a.release()


# ---- at size
def at_size(zk, k):
    h2, capi = zk.halo2, zk._capi
    lib, ptr = capi.lib(), capi.ptr
    n = 1 << k
    g = torch.empty(n * 64, dtype=torch.uint8, device="cuda"); gl = torch.empty(n * 64, dtype=torch.uint8, device="cuda")
    w = pow(h2.FR_ROOT_OF_UNITY, 1 << (h2.FR_S - k), h2.R_MOD)
    capi.check(lib.mi355_srs_setup_dev(ptr(g), ptr(gl), k, ptr(h2.fr(TAU + k)), ptr(h2.fr(w))))
    del g
    words = h2.g1_compress(gl)
    back = h2.g1_decompress(words)
    torch.cuda.synchronize()
    assert torch.equal(back, gl), "decompress(compress(P)) == P on the device"
    assert hashlib.sha256(back.cpu().numpy()).hexdigest() == hashlib.sha256(gl.cpu().numpy()).hexdigest()
    # the words against the oracle on a sample
    host = words.cpu().numpy().reshape(n, 32); pts = gl.cpu().numpy().view(np.uint64).reshape(n, 8)
    for i in list(range(0, n, n // 64)) + [n - 1]:
        assert host[i].tobytes() == cref.g1_compress(pts[i])


def test_codec_at_2_pow_24(zk):
    at_size(zk, 24)


def test_codec_at_2_pow_26(zk):
    capi = zk._capi
    free = C.c_uint64()
    capi.check(capi.lib().mi355_buf_trim())
    torch.cuda.empty_cache()
    capi.check(capi.lib().mi355_mem_info(0, C.byref(free), None, None, None, None))
    need = 12 << 30   # two bases while the set-up runs (8 GiB) + its workspace; then one basis, its words (2 GiB) and the decompressed copy (4 GiB, in the freed basis's place)
    if free.value < need:
        pytest.skip(f"2^26 needs about {need >> 30} GiB of device memory, {free.value / 2**30:.1f} GiB are free")
    at_size(zk, 26)


def test_compiled_caller(zk):
    exe = ge.build_cpp("test_g1_codec")
    zk.shutdown()
    try:
        r = subprocess.run([exe, "14"], capture_output=True, text=True, timeout=600)
    finally:
        zk.init(0)
    assert r.returncode == 0, r.stdout + r.stderr
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert rec["ok"] is True and rec["k"] == 14 and rec["load_processed_ms"] > 0 and rec["load_raw_ms"] > 0
