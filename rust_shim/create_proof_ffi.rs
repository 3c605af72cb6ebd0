//! create_proof_ffi.rs -- tier C WITHOUT a transcription: the fork of `halo2_proofs` calls the C++ prover of include/mi355zk_plonk.hpp through the
//! `mi355_plonk_*` entry points of include/mi355zk.h (bound in rust_shim/mi355zk.rs) instead of re-stating its flow in Rust, as
//! rust_shim/create_proof_resident.rs does.  One FFI call proves; what runs behind it is the code whose proof bytes equal the CPU restatement of halo2's
//! create_proof in every tested configuration (tests/test_plonk_protocol.py, tests/test_gpu_plonk_capi.py).
//!
//! NOT compiled here (no rustc / cargo in this repository's container); tests/test_shim_matches_header.py holds the `extern "C"` lines it uses to the header.
//!
//! What the fork still supplies, and where it has it:
//!   the protocol       snark-verifier's `compile(params, vk, Config::kzg()...)` serialised with serde_json: the same PlonkProtocol the prover crate writes
//!                      next to every proof [REF release-v0.13.1/chunk.protocol]
//!   the fixed columns  `Assembly::fixed` of keygen, one call per column ("preprocessed", index = the column's position among the protocol's preprocessed
//!                      polynomials); the sigma columns are NOT passed -- they follow from the copy pairs
//!   the copy pairs     `permutation::keygen::Assembly::copy` calls, as (position, row, position, row) with positions in the permutation's column order
//!   the advice columns `WitnessCollection::advice` after synthesis, the instance values, and for the mv-lookups either the `m` columns or nothing at all
//!                      (option device_multiplicities = 1: the library counts them after theta)
//!   the randomness     either the blinding parts ("m_blind", "z_blind", "phi_blind", "random_poly", and the last `blind` rows of every advice column) drawn
//!                      from the rng create_proof is handed, or ONE 32-byte key (options device_randomness = 1, rng_key = hex): the device draws everything
//! Everything else -- commitments, transforms, the quotient, the evaluations, SHPLONK, the transcript -- happens inside the one call.
#![allow(dead_code)]
use std::ffi::{CStr, CString};
use std::os::raw::{c_char, c_void};

use crate::mi355zk::*;

#[derive(Debug)]
pub struct Error { pub code: i32, pub message: String }
fn check(rc: i32) -> Result<(), Error> {
    if rc == MI355_OK { return Ok(()); }
    let message = unsafe { CStr::from_ptr(mi355_last_error()) }.to_string_lossy().into_owned();
    Err(Error { code: rc, message })
}
fn cstr(s: &str) -> CString { CString::new(s).expect("no NUL inside a name") }

/// One library object (protocol, circuit, proving key, options, record); `Drop` frees the handle.  A circuit and a key keep their protocol alive inside
/// the library, so the drop order does not matter.  An object is used by one thread at a time (`&mut self` where the library writes).
pub struct Handle(pub u64);
impl Drop for Handle { fn drop(&mut self) { if self.0 != 0 { unsafe { let _ = mi355_plonk_free(self.0); } } } }

pub fn protocol_from_json(json: &str) -> Result<Handle, Error> {
    let mut h = 0u64;
    check(unsafe { mi355_plonk_protocol_from_json(json.as_ptr() as *const c_char, json.len() as u64, &mut h) })?;
    Ok(Handle(h))
}
pub fn protocol_info(protocol: &Handle, field: &str) -> Result<u64, Error> {
    let mut v = 0u64;
    check(unsafe { mi355_plonk_protocol_info(protocol.0, cstr(field).as_ptr(), &mut v) })?;
    Ok(v)
}
pub fn circuit_new(protocol: &Handle) -> Result<Handle, Error> {
    let mut h = 0u64;
    check(unsafe { mi355_plonk_circuit_new(protocol.0, &mut h) })?;
    Ok(Handle(h))
}
/// `what`: preprocessed | advice | m | m_counts | m_blind | z_blind | phi_blind | random_poly | instances | copies.  `data` is the column as it sits in memory
/// (`&[Fr]`: 32-byte Montgomery words, the layout asserted in mi355zk::available()); sizes are checked against the protocol.
pub fn circuit_set<T>(circuit: &mut Handle, what: &str, index: u32, data: &[T]) -> Result<(), Error> {
    check(unsafe { mi355_plonk_circuit_set(circuit.0, cstr(what).as_ptr(), index, data.as_ptr() as *const c_void, std::mem::size_of_val(data) as u64) })
}
pub fn options(pairs: &[(&str, &str)]) -> Result<Handle, Error> {
    let mut h = 0u64;
    check(unsafe { mi355_plonk_options_new(&mut h) })?;
    let o = Handle(h);
    for (name, value) in pairs { check(unsafe { mi355_plonk_options_set(o.0, cstr(name).as_ptr(), cstr(value).as_ptr()) })?; }
    Ok(o)
}
/// keygen_vk + keygen_pk: the key stays resident in HBM until the handle drops.  `srs_g_lagrange`: `params.gpu_g_lagrange` (GpuBasis.0).
pub fn keygen(protocol: &Handle, circuit: &Handle, srs_g_lagrange: u64, resident_cosets: bool) -> Result<Handle, Error> {
    let mut h = 0u64;
    check(unsafe { mi355_plonk_keygen(protocol.0, circuit.0, srs_g_lagrange, resident_cosets as u32, 1, &mut h) })?;
    Ok(Handle(h))
}
pub fn vk_bytes(pk: &Handle) -> Result<Vec<u8>, Error> {
    let mut n = 0u64;
    check(unsafe { mi355_plonk_pk_vk(pk.0, std::ptr::null_mut(), 0, &mut n) })?;
    let mut out = vec![0u8; n as usize];
    check(unsafe { mi355_plonk_pk_vk(pk.0, out.as_mut_ptr() as *mut c_void, n, &mut n) })?;
    Ok(out)
}
fn record_json(record: u64) -> Result<String, Error> {
    let r = Handle(record);
    let mut n = 0u64;
    check(unsafe { mi355_plonk_record_json(r.0, std::ptr::null_mut(), 0, &mut n) })?;
    let mut out = vec![0u8; n as usize];
    check(unsafe { mi355_plonk_record_json(r.0, out.as_mut_ptr() as *mut c_char, n, &mut n) })?;
    Ok(String::from_utf8_lossy(&out).into_owned())
}
/// halo2_proofs::plonk::create_proof: the proof bytes the transcript writer would hold, and the library's record of the run (JSON: step times, counts).
/// With the option check_witness = 1 a witness that breaks a constraint is `Err` (MI355_EBADARG) naming the first failure -- halo2's MockProver, on the device.
pub fn create_proof(srs_g: u64, srs_g_lagrange: u64, pk: &Handle, circuit: &Handle, opts: Option<&Handle>, evm_layout: bool, protocol: &Handle) -> Result<(Vec<u8>, String), Error> {
    let cap = protocol_info(protocol, if evm_layout { "proof_bytes_evm" } else { "proof_bytes_poseidon" })?;
    let mut proof = vec![0u8; cap as usize];
    let (mut n, mut record) = (0u64, 0u64);
    check(unsafe { mi355_plonk_create_proof(srs_g, srs_g_lagrange, pk.0, circuit.0, opts.map_or(0, |o| o.0), proof.as_mut_ptr() as *mut c_void, cap, &mut n, &mut record) })?;
    proof.truncate(n as usize);
    Ok((proof, record_json(record)?))
}
/// The verifier of [REF integration/src/prove.rs:50-53,75-80] over one proof: accepted or the named failure.  `instances`: `&[Fr]`; `g2`, `s_g2`: the 128-byte
/// G2Affine values of ParamsKZG.
pub fn verify_proof(protocol: &Handle, vk: &[u8], instances: &[[u64; 4]], proof: &[u8], g2: &[u8; 128], s_g2: &[u8; 128], opts: Option<&Handle>) -> Result<(bool, String), Error> {
    let (protocols, vks, vk_len) = ([protocol.0], [vk.as_ptr() as *const c_void], [vk.len() as u64]);
    let (ins, n_ins) = ([instances.as_ptr() as *const c_void], [instances.len() as u64]);
    let (proofs, proof_len) = ([proof.as_ptr() as *const c_void], [proof.len() as u64]);
    let (mut ok, mut record) = ([0u8; 1], 0u64);
    check(unsafe {
        mi355_plonk_verify_proofs(1, protocols.as_ptr(), vks.as_ptr(), vk_len.as_ptr(), ins.as_ptr(), n_ins.as_ptr(), proofs.as_ptr(), proof_len.as_ptr(),
                                  g2.as_ptr() as *const c_void, s_g2.as_ptr() as *const c_void, 0, opts.map_or(0, |o| o.0), 1, ok.as_mut_ptr(), &mut record)
    })?;
    Ok((ok[0] == 1, record_json(record)?))
}

/// The short flow.  `fixed[i]`: (index among the protocol's preprocessed polynomials, column); `copies`: [position a, row a, position b, row b];
/// `rng_key`: 32 bytes from the rng create_proof was handed (`rng.fill_bytes`), ONE per proof, as secret as the witness.
pub fn prove_layer(protocol_json: &str, fixed: &[(u32, &[[u64; 4]])], copies: &[[u64; 4]], advice: &[&[[u64; 4]]], instances: &[[u64; 4]], rng_key: &[u8; 32],
                   srs_g: u64, srs_g_lagrange: u64, g2: &[u8; 128], s_g2: &[u8; 128]) -> Result<(Vec<u8>, Vec<u8>), Error> {
    let protocol = protocol_from_json(protocol_json)?;
    let mut circuit = circuit_new(&protocol)?;
    for (index, column) in fixed { circuit_set(&mut circuit, "preprocessed", *index, column)?; }
    circuit_set(&mut circuit, "copies", 0, copies)?;
    circuit_set(&mut circuit, "instances", 0, instances)?;
    let pk = keygen(&protocol, &circuit, srs_g_lagrange, true)?;                  // once per circuit: keep `pk` (and `protocol`) for every later proof
    for (a, column) in advice.iter().enumerate() { circuit_set(&mut circuit, "advice", a as u32, column)?; }
    let key_hex: String = rng_key.iter().map(|b| format!("{:02x}", b)).collect();
    let opts = options(&[("device_multiplicities", "1"), ("device_randomness", "1"), ("rng_key", &key_hex)])?;
    let evm = protocol_info(&protocol, "layer")? == 6;
    let (proof, _record) = create_proof(srs_g, srs_g_lagrange, &pk, &circuit, Some(&opts), evm, &protocol)?;
    let vk = vk_bytes(&pk)?;
    let (accepted, record) = verify_proof(&protocol, &vk, instances, &proof, g2, s_g2, None)?;
    if !accepted { return Err(Error { code: 1, message: record }); }
    Ok((proof, vk))
}
