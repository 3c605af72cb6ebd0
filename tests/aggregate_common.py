"""TEST INFRASTRUCTURE: KzgAs::create_proof restated with Python integers [EXT-recalled snark-verifier pcs/kzg/accumulation.rs], the independent statement plonk::aggregate is
held to.  Built on oracle.plonk.PoseidonTranscript and oracle.pyref alone:
  accumulators(verdicts)   proof i gives (msm result_i, W'_i); a proof that carries an accumulator in its first twelve instances gives that one AFTER it
  challenge(accs)          a fresh Poseidon transcript, no initial scalar, absorbs lhs then rhs of every accumulator in list order; r = one squeeze
  fold(accs, r)            (sum r^j lhs_j, sum r^j rhs_j), r^0 = 1
  limbs(lhs, rhs)          three 88-bit limbs per coordinate: lhs.x, lhs.y, rhs.x, rhs.y
No fixture pins r: the order and the transcript are recalled.  What these helpers let the tests verify is the algebra."""
from oracle import plonk, pyref

R, P = pyref.R_MOD, pyref.P_MOD
LIMB = (1 << 88) - 1


def carried(instances):
    """the accumulator in the first twelve instances: ((lhs.x, lhs.y), (rhs.x, rhs.y))"""
    c = [int(instances[3 * i]) + (int(instances[3 * i + 1]) << 88) + (int(instances[3 * i + 2]) << 176) for i in range(4)]
    return (c[0], c[1]), (c[2], c[3])


def accumulators(verdicts, instance_lists, carries):
    """verdicts: oracle.plonk.verify() dictionaries (their msm.result and msm.w_prime); carries[i]: proof i carries an accumulator"""
    out = []
    for v, inst, has in zip(verdicts, instance_lists, carries):
        out.append((tuple(v["msm"]["result"]), tuple(v["msm"]["w_prime"])))
        if has:
            out.append(carried(inst))
    return out


def challenge(accs):
    T = plonk.PoseidonTranscript()
    for lhs, rhs in accs:
        T.common_point(lhs); T.common_point(rhs)
    return T.squeeze()


def fold(accs, r):
    lhs = rhs = None
    pw = 1
    for l, rr in accs:
        lhs = pyref.g1_add(lhs, pyref.g1_mul(l, pw)); rhs = pyref.g1_add(rhs, pyref.g1_mul(rr, pw))
        pw = pw * r % R
    return lhs, rhs


def limbs(lhs, rhs):
    return [(c >> (88 * l)) & LIMB for c in (lhs[0], lhs[1], rhs[0], rhs[1]) for l in range(3)]


# ---- the released proofs as cases of halo2.verify_proofs / halo2.aggregate, and the oracle's verdict on each (computed once per process, never modified)
import functools

from verify_common import ALL_TEN, case, oracle_verify, product_protocol

SEVEN = ALL_TEN[:7]                      # the seven chunk proofs (layer 2)


def product_case(name, inst=None, proof=None, **over):
    """one entry of the list halo2.verify_proofs takes; inst / proof / keywords replace the released ones"""
    layer, i0, p0, _, pkw = case(name)
    return dict(dict(pkw, **over), protocol=product_protocol(layer), instances=list(i0 if inst is None else inst), proof=bytes(p0 if proof is None else proof))


@functools.lru_cache(maxsize=None)
def oracle_verdict(name):
    layer, inst, proof, okw, _ = case(name)
    return oracle_verify(layer, inst, proof, okw)


def restated(names):
    """-> (accumulators, r) of the released proofs `names` by the helpers above: every one of them carries an accumulator"""
    accs = accumulators([oracle_verdict(n) for n in names], [case(n)[1] for n in names], [True] * len(names))
    return accs, challenge(accs)
