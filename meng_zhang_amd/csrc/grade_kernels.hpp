// grade_kernels.hpp -- the extrapolation guard (annp_hip_set_extrapolation): how far outside the training range of the
// potential does each atom's descriptor lie?
//
// For list entry ii the grade is  max_k |G[ii][k] - c_k| / w_k  over the features the potential has; c and w come from the
// training statistics in the potential file (Behler: the middle and half the width of [sf_min, sf_max], so grade <= 1 means every
// function inside its range; Chebyshev: average and standard deviation, so the grade is the largest |z-score|) or from the caller.
// The reference has no such guard.
//
// One pass over the descriptor rows an evaluation leaves in G (ANNP_GPAD = 32 doubles per entry): 256 bytes in, 9 bytes out per
// entry, no arithmetic to speak of, so the kernel is shaped for the memory system.  Sixteen lanes share an entry, each lane loads one
// double2 (global_load_dwordx4): a wave's load instruction reads four whole rows, 1 KB contiguous.  Centre and 1 / width of a lane's two
// features are registers for the whole launch.  The maximum over the sixteen lanes goes through four row_shr moves (no LDS, no
// barrier) and arrives in the row's LAST lane, which writes the grade and the slot of the feature that set it (lowest slot on ties).
// The two counters -- entries above the threshold, (entry, feature) values above it -- are wave ballots added up in scalar registers;
// a workgroup adds them to the evaluation's flag words once, at its end (as annp_mlp_mfma does for the energy word).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "annp_common.hpp"

namespace annp {

constexpr int GRADE_WAVES = 4;              // waves per workgroup: 16 entries per trip of the loop
constexpr int GRADE_MAX_BLOCKS = 2048;      // 256 CUs x 8 workgroups: every wave resident, the loop strides over the rest

struct GradeArgs {
    int n;                          // list entries
    const double *G;                // [n][pitch] descriptor rows of the evaluation (pitch: ANNP_GPAD; annp_desc_grade_wide: 64)
    const double *stat;             // centre[pitch] | 1 / halfwidth[pitch] by slot of the row; 0 where no feature of the potential sits
    double threshold;
    double *grade;                  // [n]
    unsigned char *feat;            // [n] slot of the feature that set the grade
    const int *ilist, *type;        // type != null: a centre of an unmapped type has no descriptor; its grade is 0
    unsigned active;
    int *n_above, *n_values;        // flag words: entries with grade > threshold, (entry, feature) values above it
};

constexpr int GRADE_PER_BLOCK = 4 * GRADE_WAVES;        // entries per workgroup and trip: four per wave
inline int grade_blocks(int n) { return std::max(1, std::min((n + GRADE_PER_BLOCK - 1) / GRADE_PER_BLOCK, GRADE_MAX_BLOCKS)); }

template <int CTRL>
__device__ __forceinline__ int dpp_from_int(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, false); }

// (value, slot) of the larger value, the lower slot on equal values, between a lane and the lane SHR places before it in its row of 16
template <int CTRL>
__device__ __forceinline__ void grade_row_step(double &v, int &k)
{
    const double ov = dpp_from<CTRL, 0xf>(v);       // (lanes without a source read 0.0 / slot 0: never larger than a grade)
    const int ok = dpp_from_int<CTRL>(k);
    const bool take = ov > v || (ov == v && ok < k);
    v = take ? ov : v;
    k = take ? ok : k;
}

__global__ __launch_bounds__(64 * GRADE_WAVES) void annp_desc_grade(const GradeArgs p)
{
    __shared__ int part[2 * GRADE_WAVES];
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const int l = lane & 15, row = lane >> 4;
    const double2 c = reinterpret_cast<const double2 *>(p.stat)[l];
    const double2 iw = reinterpret_cast<const double2 *>(p.stat + ANNP_GPAD)[l];
    const double thr = p.threshold;
    int n_above = 0, n_values = 0;          // wave-uniform
    for (int base = (blockIdx.x * GRADE_WAVES + wave) * 4; base < p.n; base += gridDim.x * GRADE_PER_BLOCK) {
        const int ii = base + row;
        bool live = ii < p.n;
        if (live && p.type) live = type_mapped(p.active, p.type[p.ilist ? p.ilist[ii] : ii]);
        double d0 = 0.0, d1 = 0.0;
        if (live) {
            const double2 g = reinterpret_cast<const double2 *>(p.G + (size_t)ii * ANNP_GPAD)[l];
            d0 = fabs(g.x - c.x) * iw.x;
            d1 = fabs(g.y - c.y) * iw.y;
        }
        n_values += __popcll(__ballot(d0 > thr)) + __popcll(__ballot(d1 > thr));
        double v = d1 > d0 ? d1 : d0;
        int k = 2 * l + (d1 > d0 ? 1 : 0);
        grade_row_step<0x111>(v, k);        // row_shr:1
        grade_row_step<0x112>(v, k);        // row_shr:2
        grade_row_step<0x114>(v, k);        // row_shr:4
        grade_row_step<0x118>(v, k);        // row_shr:8 -> the row's last lane has looked at all sixteen
        const bool writer = l == 15 && ii < p.n;
        if (writer) {
            p.grade[ii] = v;
            p.feat[ii] = (unsigned char)k;
        }
        n_above += __popcll(__ballot(writer && v > thr));
    }
    if (lane == 0) { part[2 * wave] = n_above; part[2 * wave + 1] = n_values; }
    __syncthreads();
    if (threadIdx.x == 0) {
        int a = 0, b = 0;
#pragma unroll
        for (int w = 0; w < GRADE_WAVES; w++) { a += part[2 * w]; b += part[2 * w + 1]; }
        if (a) atomicAdd(p.n_above, a);
        if (b) atomicAdd(p.n_values, b);
    }
}

// The same pass over rows of 64 doubles (the wide Behler route, ni_wide_kernels.hpp): sixteen lanes still share an entry, each lane now
// looks at slots 2l, 2l+1 and 32+2l, 32+2l+1 (two double2 loads: a wave's two load instructions read four whole rows of 512 bytes).
// `stat` is centre[64] | 1 / halfwidth[64].  Same outputs, same counters, same tie rule (the lowest slot).
constexpr int GRADE_WIDE_PITCH = 64;

__global__ __launch_bounds__(64 * GRADE_WAVES) void annp_desc_grade_wide(const GradeArgs p)
{
    __shared__ int part[2 * GRADE_WAVES];
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const int l = lane & 15, row = lane >> 4;
    const double2 c0 = reinterpret_cast<const double2 *>(p.stat)[l], c1 = reinterpret_cast<const double2 *>(p.stat)[16 + l];
    const double2 iw0 = reinterpret_cast<const double2 *>(p.stat + GRADE_WIDE_PITCH)[l], iw1 = reinterpret_cast<const double2 *>(p.stat + GRADE_WIDE_PITCH)[16 + l];
    const double thr = p.threshold;
    int n_above = 0, n_values = 0;          // wave-uniform
    for (int base = (blockIdx.x * GRADE_WAVES + wave) * 4; base < p.n; base += gridDim.x * GRADE_PER_BLOCK) {
        const int ii = base + row;
        bool live = ii < p.n;
        if (live && p.type) live = type_mapped(p.active, p.type[p.ilist ? p.ilist[ii] : ii]);
        double d[4] = {0.0, 0.0, 0.0, 0.0};
        if (live) {
            const double2 *g = reinterpret_cast<const double2 *>(p.G + (size_t)ii * GRADE_WIDE_PITCH);
            const double2 g0 = g[l], g1 = g[16 + l];
            d[0] = fabs(g0.x - c0.x) * iw0.x; d[1] = fabs(g0.y - c0.y) * iw0.y;
            d[2] = fabs(g1.x - c1.x) * iw1.x; d[3] = fabs(g1.y - c1.y) * iw1.y;
        }
        double v = d[0];
        int k = 2 * l;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            n_values += __popcll(__ballot(d[q] > thr));
            const int slot = 2 * l + (q & 1) + 32 * (q >> 1);
            if (d[q] > v) { v = d[q]; k = slot; }       // (slots ascend with q: the lowest slot stays on ties)
        }
        grade_row_step<0x111>(v, k);
        grade_row_step<0x112>(v, k);
        grade_row_step<0x114>(v, k);
        grade_row_step<0x118>(v, k);
        const bool writer = l == 15 && ii < p.n;
        if (writer) {
            p.grade[ii] = v;
            p.feat[ii] = (unsigned char)k;
        }
        n_above += __popcll(__ballot(writer && v > thr));
    }
    if (lane == 0) { part[2 * wave] = n_above; part[2 * wave + 1] = n_values; }
    __syncthreads();
    if (threadIdx.x == 0) {
        int a = 0, b = 0;
#pragma unroll
        for (int w = 0; w < GRADE_WAVES; w++) { a += part[2 * w]; b += part[2 * w + 1]; }
        if (a) atomicAdd(p.n_above, a);
        if (b) atomicAdd(p.n_values, b);
    }
}

}  // namespace annp
