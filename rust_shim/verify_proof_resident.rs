//! verify_proof_resident.rs -- the device route of `verify_proof::<KZGCommitmentScheme<Bn256>, VerifierSHPLONK<'_, Bn256>, _, _, _>` as Rust, against the
//! `extern "C"` block of rust_shim/mi355zk.rs.  It goes next to `halo2_proofs/src/plonk/verifier.rs` in the fork of scroll-tech/halo2 @ e5ddf67
//! [REF Cargo.lock:1886-1888]; the reference reaches it from `prove_and_verify_chunk` / `_batch` / `_bundle` [REF integration/src/prove.rs:23-107].
//!
//! NOT compiled and NEVER TYPE-CHECKED: this repository's container has no rustc / cargo.  It is the twin of
//! `mi355zk::plonk::verify_proof` in include/mi355zk_plonk_verify.hpp, which IS compiled and run (tests/cpp/test_verify_proof.cpp,
//! tests/test_verify_proof_surface.py, `pytest -m gpu tests/test_gpu_verify_proof.py`) and accepts the reference's ten released proofs under the released -[s]G2.
//! tests/test_shim_matches_header.py holds the extern block to include/mi355zk.h.
//!
//! A sketch of the CALL SITE, thinner than create_proof_resident.rs on purpose: the flow around these calls is halo2's own verifier.rs unchanged (its transcript and its
//! `Expression::evaluate` already do what the C++ twin restates for a PlonkProtocol JSON), so only the three points where the fork leaves the CPU are written out.
//! What stays in verifier.rs: the transcript (`read_point` / `read_scalar` / `squeeze_challenge` on the host), the evaluation of the expression graph at x and the
//! scalar side of SHPLONK -- field arithmetic on a few hundred values.  What moves to the device: the decompression of the proof's points (one call), the verifier's one
//! multi-scalar multiplication (one call) and the pairing (one call).
#![allow(dead_code)]
use std::os::raw::c_void;

use halo2curves::bn256::{Fr, G1Affine, G2Affine, G1};

use crate::mi355zk;

/// The two G2 points of the final check, as the pairing takes them (hpp: `G2Pair`): g2 and -[s]g2.
pub struct G2Pair { pub g2: G2Affine, pub neg_s_g2: G2Affine }
impl G2Pair {
    /// from `ParamsKZG`'s `g2` / `s_g2`: s_g2 is negated on the host
    pub fn from_params(g2: G2Affine, s_g2: G2Affine) -> Self { G2Pair { g2, neg_s_g2: -s_g2 } }
}

/// hpp: step "every compressed point word of the proof through one decompression".  `words`: the 32-byte words at the positions the protocol fixes
/// (num_witness + Q commitments, then the two SHPLONK points behind the evaluations).  Err(i): word i is no curve point.
pub fn decompress_proof_points(words: &[[u8; 32]]) -> Result<Vec<G1Affine>, u64> {
    let mut out = vec![G1Affine::default(); words.len()];
    let mut bad = u64::MAX;
    let rc = unsafe { mi355zk::mi355_g1_decompress_host(words.as_ptr() as *const c_void, out.as_mut_ptr() as *mut c_void, words.len() as u64, &mut bad) };
    if rc == 0 { Ok(out) } else { Err(bad) }
}

/// hpp: "one MSM".  The (scalars, points) list SHPLONK collapses to: sum_p coeff_p C_p, the quotient's commitment spread over its pieces with x^(n q), the
/// generator with -r, C_H with -Z_T(u) / zd_0, W' with u.
pub fn msm_lhs(scalars: &[Fr], points: &[G1Affine]) -> Result<G1, i32> {
    assert_eq!(scalars.len(), points.len());
    let mut out = G1::default();
    let rc = unsafe { mi355zk::mi355_msm_g1_adhoc_host(points.as_ptr() as *const c_void, scalars.as_ptr() as *const c_void, scalars.len() as u64, &mut out as *mut G1 as *mut c_void) };
    if rc == 0 { Ok(out) } else { Err(rc) }
}

/// hpp: "one pairing call".  Group 0 = e(lhs, g2) e(W', -s_g2); group 1, when the circuit carries an accumulator (`accumulator_indices`: twelve 88-bit limbs in the
/// first instances, both points checked on the curve by the caller), = e(acc.lhs, g2) e(acc.rhs, -s_g2).  Returns the per-group verdicts.
pub fn pairing_check(lhs: G1Affine, w_prime: G1Affine, accumulator: Option<(G1Affine, G1Affine)>, srs: &G2Pair) -> Result<Vec<bool>, i32> {
    let mut p = vec![lhs, w_prime];
    if let Some((l, r)) = accumulator { p.push(l); p.push(r); }
    let groups = (p.len() / 2) as u32;
    let q: Vec<G2Affine> = (0..groups).flat_map(|_| [srs.g2, srs.neg_s_g2]).collect();
    let mut one = vec![0u32; groups as usize];
    let rc = unsafe { mi355zk::mi355_pairing_products_host(p.as_ptr() as *const c_void, q.as_ptr() as *const c_void, groups, 2, std::ptr::null_mut(), one.as_mut_ptr()) };
    if rc == 0 { Ok(one.into_iter().map(|f| f == 1).collect()) } else { Err(rc) }
}

/// `ParamsKZG::check_g2` (hpp: include/mi355zk_halo2.hpp): e(g[0], s_g2) e(-g[1], g2) == 1
pub fn check_g2(g0: G1Affine, g1: G1Affine, g2: G2Affine, s_g2: G2Affine) -> Result<bool, i32> {
    let p = [g0, -g1]; let q = [s_g2, g2]; let mut one = 0u32;
    let rc = unsafe { mi355zk::mi355_pairing_products_host(p.as_ptr() as *const c_void, q.as_ptr() as *const c_void, 1, 2, std::ptr::null_mut(), &mut one) };
    if rc == 0 { Ok(one == 1) } else { Err(rc) }
}
