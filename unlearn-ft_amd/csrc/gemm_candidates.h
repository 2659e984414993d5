// Internal interface of the GEMM family (gemm.hip, gemm_dma.hip, gemm_ring.hip, gemm_rowblock.hip): the cross-file launch /
// name functions and the candidate numbering.  Not part of the C ABI (include/pdmk.h).
//
// Candidate ids are what plan files, the tuner, tests and tools name kernels by, and they are stable.  Id 0 = the K-step-32
// kernels (gemm.hip / gemm_dma.hip); candidate id c >= 1 is "ring id" c - 1 of the pdmk_gemm_ring_* (forward / dgrad) or
// pdmk_wgrad_ring_* (weight gradient, a_mode = PDMK_A_COLK) functions below.  Ring ids of both families have one layout: the
// first `base` ring shapes, the halo shapes, the ring shapes added later, and (forward only) the row-block kernels.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/pdmk.h"

// All launch functions return 0 = launched, 1 = this candidate does not serve the problem (the caller falls back),
// -1000 = launch error.  a_bytes / b_bytes: extent of the operands (buffer descriptors).
int pdmk_gemm_dma_launch(const pdmk_gemm_args& g, hipStream_t st, long a_bytes, long b_bytes);                        // gemm_dma.hip
void pdmk_gemm_note_form(int form);                                  // gemm.hip: what pdmk_gemm_last_form() reports (pdmk.h)
int pdmk_gemm_ring_launch(const pdmk_gemm_args& g, hipStream_t st, long a_bytes, long b_bytes, int id);               // gemm_ring.hip
int pdmk_gemm_ring_group_launch(const pdmk_gemm_args* gs, int n, hipStream_t st, const long* a_bytes, const long* b_bytes, int id);
int pdmk_gemm_ring_num_configs();                                    // ring + halo + row-block ids
int pdmk_gemm_ring_pick(const pdmk_gemm_args& g);                    // untuned default (ring id)
int pdmk_gemm_ring_name(int id, int conv, char* buf, int n);
int pdmk_wgrad_ring_launch(const pdmk_gemm_args& g, hipStream_t st, long a_bytes, long b_bytes, int id);
int pdmk_wgrad_ring_group_launch(const pdmk_gemm_args* gs, int n, hipStream_t st, const long* a_bytes, const long* b_bytes, int id);
int pdmk_wgrad_ring_num_configs();                                   // ring + halo ids
int pdmk_wgrad_ring_name(int id, int conv, char* buf, int n);
int pdmk_gemm_rowblock_launch(const pdmk_gemm_args& g, hipStream_t st, long a_bytes, long b_bytes, int id, bool dry = false);   // gemm_rowblock.hip
int pdmk_gemm_rowblock_num_configs();
int pdmk_gemm_rowblock_name(int id, char* buf, int n);

namespace pdmk_cand {

enum Family { NONE, RING, HALO, ROWBLOCK };
struct Ref {
    Family fam;
    int row;          // row of that family's table
};
// ring id -> (family, table row) for a family with `base` ring rows in front of `nhalo` halo rows, `nring` ring rows in all
// and `nrb` row-block rows at the end
inline Ref decode(int id, int base, int nhalo, int nring, int nrb) {
    if (id < 0) return {NONE, 0};
    if (id < base) return {RING, id};
    if (id < base + nhalo) return {HALO, id - base};
    if (id < nring + nhalo) return {RING, id - nhalo};
    if (id < nring + nhalo + nrb) return {ROWBLOCK, id - nring - nhalo};
    return {NONE, 0};
}

// ring ids (fixed by the plan files in the field: later ring shapes go BEHIND the halo ids)
constexpr int kRingBase = 12, kHaloCount = 4;              // forward / dgrad
constexpr int kWgradRingBase = 5, kWgradHaloCount = 2;     // weight gradients

// candidate ids
constexpr int kHaloFirst = 1 + kRingBase;                  // .. kHaloFirst + kHaloCount - 1: the halo-conv shapes
constexpr int kWgradRingCount = kWgradRingBase;            // 1 .. kWgradRingCount: the weight-gradient ring shapes
constexpr int kWgradHaloFirst = 1 + kWgradRingBase;        // .. + kWgradHaloCount - 1: the halo conv weight gradients
constexpr int kWgradHeuristic = 2;                         // untuned conv weight gradients: the shallow 128 x 128 ring
inline int rowblock_first() { return 1 + pdmk_gemm_ring_num_configs() - pdmk_gemm_rowblock_num_configs(); }

}  // namespace pdmk_cand
