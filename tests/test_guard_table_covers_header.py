"""every declaration of include/mi355zk.h that takes a device pointer has a row in the guard-band sweep (tests/test_gpu_guard_bands.py TABLE) or stands in EXEMPT with its
reason.  The next entry point that is added without a guard case fails here, on a machine without a GPU."""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.test_shim_matches_header import _strip_c_comments

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the three entry points of the device randomness name their device operands dst / cols / src: the header documents them as device memory ("asynchronous on the library
# stream of the device that owns the destination", "cols: host array of n_cols device pointers")
DOCUMENTED_DEVICE_PARAMS = {"mi355_fr_random_dev": ["dst"], "mi355_fr_random_rows_dev": ["cols"], "mi355_fr_from_u512_dev": ["dst", "src"]}

# what the sweep leaves out, each with its reason: entry points that take host pointers stage their own device memory; allocation, release and handle calls have no operand range
EXEMPT = {}


def device_pointer_declarations():
    """name -> the parameters that are device pointers: every parameter named *_dev, and the documented ones above"""
    src = _strip_c_comments(open(os.path.join(ROOT, "include", "mi355zk.h")).read())
    out = {}
    for m in re.finditer(r"(?:^|\n)\s*(?:const\s+)?\w+\s*\**\s*(mi355_\w+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S):
        name, args = m.group(1), " ".join(m.group(2).split())
        names = [re.match(r"^.*?(\w+)$", a.strip()).group(1) for a in args.split(",")] if args and args != "void" else []
        dev = [p for p in names if p.endswith("_dev")] + [p for p in DOCUMENTED_DEVICE_PARAMS.get(name, []) if p in names]
        if dev:
            out[name] = dev
    return out


def test_the_parser_sees_the_device_pointer_surface():
    decl = device_pointer_declarations()
    assert len(decl) >= 46, sorted(decl)
    assert decl["mi355_fr_kate_division_dev"] == ["dst_dev", "poly_dev"]
    assert decl["mi355_coset_ntt_fr_batch_dev"] == ["dst_dev", "coeffs_dev"]
    assert decl["mi355_fr_from_u512_dev"] == ["dst", "src"]
    assert decl["mi355_buf_upload"] == ["dst_dev"] and decl["mi355_msm_g2_dev"] == ["bases_g2affine_dev", "scalars_dev"]
    assert "mi355_msm_g1_host" not in decl and "mi355_buf_alloc" not in decl and "mi355_plonk_create_proof" not in decl
    for name, params in DOCUMENTED_DEVICE_PARAMS.items():
        assert decl[name] == params, name


def test_every_device_pointer_declaration_is_swept_or_exempt_with_a_reason():
    from tests.test_gpu_guard_bands import TABLE
    decl = device_pointer_declarations()
    for name in sorted(decl):
        assert (name in TABLE) != (name in EXEMPT), "%s takes device pointers (%s): give it a row in tests/test_gpu_guard_bands.py" % (name, ", ".join(decl[name]))
    for name, reason in EXEMPT.items():
        assert name in decl and len(reason) > 20, name
    stale = sorted(set(TABLE) - set(decl))
    assert not stale, "rows for entry points the header does not declare with device pointers: %s" % stale
    for name, (sizes, fn) in TABLE.items():
        assert sizes and callable(fn), name
