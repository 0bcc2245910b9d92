// split_bf16.h -- the arithmetic of the split-precision ("bf16x3") MFMA GEMMs and the bf16 vector types they share: gemm3.h
// (rollout forward, policy.hip), gemm3p.h and gemm3_tn.h (PPO update, linear.hip).  hh_fused.hip computes the same way.
#pragma once

namespace {

// ---- split-precision GEMM: fp32 operands as (hi + lo) bf16 pairs, three bf16 MFMAs per product term ------------------
// a*b ~= a_hi*b_hi + a_hi*b_lo + a_lo*b_hi with hi = bf16(x), lo = bf16(x - hi): the dropped terms are <= 2^-16 relative,
// accumulation is fp32 (measured end-to-end error on the HH block: 1.5e-5, bar 1e-4).  Runs on v_mfma_f32_32x32x16_bf16
// (16x the fp32 MFMA rate, three passes -> 5.3x).  A is fp32 in HBM and split while it is staged into LDS
// (v_cvt_pk_bf16_f32); W is split once per weight snapshot.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

} // namespace
