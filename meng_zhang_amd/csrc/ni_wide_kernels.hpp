// ni_wide_kernels.hpp -- the "wide" Behler G2/G4 route (annp_hip_eval_path 6): descriptor pass, network pass and force pass for
// potentials larger than the tuned kernels of ni_kernels.hpp take (nsf <= 64, npsf <= 32, ntsf <= 64, nnod <= 64, any real
// zeta > 0, any lambda, any number of distinct eta), and for any Behler potential under ANNP_HIP_NI_EVAL=wide.
//
// Arithmetic restated from annp-gpu-lammps/ni/src/pair_annp.cpp ("ni:"): radial G2 ni:686-711, angular G4 ni:713-767 with the
// guard 1 + lambda cos(theta) <= 0 of ni:744-747, force assembly ni:180-203, network ni:769-867.  One radial and one angular
// cutoff, those of the first row of each block, as the reference reads them.
//
// Shape of the kernels: a descriptor row has 64 slots and a wave has 64 lanes, so LANE k OWNS FUNCTION k of the file (radial
// functions first, the file's order: no visit order, no product shape).  One wave works on one atom:
//   * both passes first filter the atom's list row into LDS records (list order; 128 at most -- more is ANNP_HIP_ENEIGHCAP through
//     the evaluation's error word, the atom is skipped): xi - xj, r, and fc / fc' of the two cutoffs.  The force pass filters again
//     instead of reading a list the descriptor pass left: the same function on the same data finds the same records, and no
//     buffer of 128 indices per atom stands between the passes;
//   * descriptor: every lane sums its own function -- radial lanes over the records, angular lanes over the in-range (j, k) pairs,
//     whose geometry (cos theta, the three cutoff factors, the sum of squares) is wave-uniform.  No reduction, no atomics: G[ii][lane];
//   * force: the derivative of function n with respect to x_j is  t1_n dcos/dx_j - t2_n d(r^2 sum)/dx_j + t3_n d(fc fc fc)/dx_j  with
//     three scalars per function and three vectors per pair, so the sum over functions is three wave sums per pair (weights
//     c_n = dE/dGhat_n / (sf_max - sf_min)_n, the row the network pass left) and the vectors are formed once.  Per-neighbour totals
//     are kept in LDS and leave with one atomic per neighbour and component;
//   * zeta: a small integer keeps a multiply ladder (square and multiply, 7 steps: exact to a few ulp like pow), anything else is
//     exp(zeta log(1 + lambda cos theta)).
// The network pass (annp_mlp_wide) is a plain one: lane = node (nnod <= 64), four atoms per trip share every weight that is
// loaded, weights and their transposes come from global memory (264 KB per element: L2-resident and shared by every workgroup;
// the MFMA operand image of a 64-64-64-64-1 network would not fit in LDS).  DESIGN.md 4.4d has the budget and what is unmeasured.
//
// LDS is static, so the compiler's report carries it: 32 KB (descriptor), 48 KB (force), 8 KB (network) per workgroup of four waves.
#pragma once
#include "annp_common.hpp"
#include "mlp_kernels.hpp"
#include "ni_kernels.hpp"

namespace annp {

constexpr int NIW_PITCH = 64;       // doubles per row of G and of coef on this route
constexpr int NIW_CAP = 128;        // in-range neighbours per atom the records hold
constexpr int NIW_WAVES = 4;        // waves per workgroup, one atom each
constexpr int NIW_MAXP = 32;        // radial functions
constexpr int NIW_MAXT = 64;        // angular functions
constexpr int NIW_MAXNOD = 64;      // nodes per hidden layer (one lane each)
constexpr int NIW_MA = 4;           // network pass: atoms per wave and trip
constexpr int NIW_MAX_BLOCKS = 2048;
constexpr int NIW_LAYER = 2 * 64 * 64;                              // network image: W_l [64][64] row-major | its transpose
constexpr int NIW_IMG = MLP_MAXL * NIW_LAYER + MLP_MAXL * 64;       // ... of every layer, then the biases [MLP_MAXL][64]; per element

struct NiWideArgs {
    int inum;
    const int *ilist;
    const double *x;
    const int *type;            // nullable [nall], with `active` (annp_common.hpp type_mapped)
    unsigned active;
    const int *numneigh;
    const long long *first;
    const int *neigh;
    int npsf, ntsf, compat;
    const double *rad;          // [npsf][3] eta, Rs, Rc (Bohr), the file's order
    const double *ang;          // [ntsf][4] eta, lambda, zeta, 2^(1-zeta), the file's order
    double rc_rad, rc_ang;      // Bohr
    double por_rad, por_ang;    // pi / rc
    double *G;                  // [inum][NIW_PITCH]
    const double *coef;         // [inum][NIW_PITCH]: c_k = dE/dGhat_k / (sf_max - sf_min)_k, the file's order
    double *f;
    double *virial;             // nullable: the table of annp_common.hpp (virial_row)
    double *vatom;              // nullable, [nall][6] accumulated
    int *ncount;                // [inum] in-range neighbours (0: the atom was skipped)
    int *errflag;
};

struct MlpWideArgs {
    int inum;
    const int *ilist;
    int nsf, nnod, nl;
    int act[MLP_MAXL];
    int act_plain;
    const double *img;          // this element's image (NIW_IMG doubles)
    const double *nsub, *nden;  // [NIW_PITCH] Ghat = (G - nsub) * nden
    const double *cmul;         // [NIW_PITCH] coef_k = cmul_k dE/dGhat_k
    const double *G;
    double *coef;
    double *eatom, *eng;
    const int *type, *map;
    unsigned active;
    int elem;
};

// Host side: the network of one element as annp_mlp_wide reads it.  W[l] row-major [d_{l+1}][d_l] as in the potential file.
inline void niw_build_image(double *img, const double *const *W, const double *const *B, int nsf, int nnod, int nl)
{
    for (int k = 0; k < NIW_IMG; k++) img[k] = 0.0;
    for (int l = 0; l < nl; l++) {
        const int nr = l == nl - 1 ? 1 : nnod, nc = l == 0 ? nsf : nnod;
        double *w = img + (size_t)l * NIW_LAYER, *wt = w + 64 * 64, *b = img + (size_t)MLP_MAXL * NIW_LAYER + 64 * l;
        for (int r = 0; r < nr; r++) {
            for (int c = 0; c < nc; c++) { w[64 * r + c] = W[l][(size_t)r * nc + c]; wt[64 * c + r] = W[l][(size_t)r * nc + c]; }
            b[r] = B[l][r];
        }
    }
}

// the records of one atom (LDS of its wave)
struct NiwRec {
    double *dx, *dy, *dz, *r;           // xi - xj and its length, Angstrom
    double *fcr, *dfcr, *fca, *dfca;    // cutoff function and derivative (per Bohr) at r, for the radial and the angular cutoff
    int *j;
};

__device__ __forceinline__ NiwRec niw_records(double *base, int *jbase)
{
    NiwRec L;
    L.dx = base; L.dy = base + NIW_CAP; L.dz = base + 2 * NIW_CAP; L.r = base + 3 * NIW_CAP;
    L.fcr = base + 4 * NIW_CAP; L.dfcr = base + 5 * NIW_CAP; L.fca = base + 6 * NIW_CAP; L.dfca = base + 7 * NIW_CAP;
    L.j = jbase;
    return L;
}

// Filters the list row of atom i into the records, in list order.  Returns the number of neighbours inside the larger cutoff; above
// NIW_CAP only the first NIW_CAP were recorded and the caller drops the atom.  Nothing is written beyond slot NIW_CAP - 1.
__device__ __forceinline__ int niw_filter(const NiWideArgs &p, int i, const NiwRec &L, int lane)
{
    const int jnum = p.numneigh[i];
    const int *row = p.neigh + p.first[i];
    const double xi = p.x[3 * (size_t)i], yi = p.x[3 * (size_t)i + 1], zi = p.x[3 * (size_t)i + 2];
    const double rcmax = fmax(p.rc_rad, p.rc_ang);
    const double rc2 = (rcmax / ANNP_CFLENGTH) * (rcmax / ANNP_CFLENGTH) * (1.0 + 1e-12);       // coarse, in A^2: the exact tests follow per function
    const unsigned long long lt = (1ull << lane) - 1ull;
    int n = 0;
    for (int base = 0; base < jnum; base += ANNP_WAVE) {
        const int jj = base + lane;
        bool in = jj < jnum;
        int j = 0;
        double dx = 0.0, dy = 0.0, dz = 0.0, rsq = 0.0;
        if (in) {
            j = row[jj] & ANNP_NEIGHMASK;
            if (p.type) in = type_mapped(p.active, p.type[j]);
        }
        if (in) {
            dx = xi - p.x[3 * (size_t)j]; dy = yi - p.x[3 * (size_t)j + 1]; dz = zi - p.x[3 * (size_t)j + 2];
            rsq = dx * dx + dy * dy + dz * dz;
            in = rsq < rc2 && rsq > 0.0;
        }
        const unsigned long long m = __ballot(in);
        const int pos = n + __popcll(m & lt);
        if (in && pos < NIW_CAP) {
            const double r = sqrt(rsq), rm = r * ANNP_CFLENGTH;
            double sn, cs;
            sincos_0_pi(fmin(rm, p.rc_rad) * p.por_rad, sn, cs);        // (beyond a cutoff the value is never used: the argument stays in [0, pi])
            L.fcr[pos] = 0.5 * (cs + 1.0); L.dfcr[pos] = -0.5 * p.por_rad * sn;
            sincos_0_pi(fmin(rm, p.rc_ang) * p.por_ang, sn, cs);
            L.fca[pos] = 0.5 * (cs + 1.0); L.dfca[pos] = -0.5 * p.por_ang * sn;
            L.dx[pos] = dx; L.dy[pos] = dy; L.dz[pos] = dz; L.r[pos] = r; L.j[pos] = j;
        }
        n += __popcll(m);
    }
    wave_lds_sync();
    return uniform(n);
}

// (1 + lambda cos theta)^zeta for a positive base: the ladder for zeta = 1..64 (iz), exp(zeta log) otherwise (iz = 0)
__device__ __forceinline__ double niw_pow(double base, double zeta, int iz)
{
    if (iz > 0) {
        double res = 1.0, b = base;
#pragma unroll
        for (int bit = 0; bit < 7; bit++) {
            res = (iz >> bit) & 1 ? res * b : res;
            b *= b;
        }
        return res;
    }
    return exp(zeta * log(base));
}

__device__ __forceinline__ int niw_zeta_int(double zeta)
{
    return (zeta >= 1.0 && zeta <= 64.0 && zeta == floor(zeta)) ? (int)zeta : 0;
}

// what a (j, k) pair of records means to every function: wave-uniform
struct NiwPair {
    double ra, rb, rjk;             // Angstrom
    double rma, rmb, rmjk;          // Bohr
    double ct, fcjk, dfcjk, term_fc, r2sum;
    double ja[3], kb[3];            // xi - xj, xi - xk
};

// false: the pair is out of the angular range (ni:729)
__device__ __forceinline__ bool niw_pair(const NiWideArgs &p, const NiwRec &L, int a, int b, NiwPair &q)
{
    q.ja[0] = L.dx[a]; q.ja[1] = L.dy[a]; q.ja[2] = L.dz[a];
    q.kb[0] = L.dx[b]; q.kb[1] = L.dy[b]; q.kb[2] = L.dz[b];
    q.ra = L.r[a]; q.rb = L.r[b];
    q.rma = q.ra * ANNP_CFLENGTH; q.rmb = q.rb * ANNP_CFLENGTH;
    const double gx = q.kb[0] - q.ja[0], gy = q.kb[1] - q.ja[1], gz = q.kb[2] - q.ja[2];       // xj - xk
    const double r2jk = gx * gx + gy * gy + gz * gz;
    q.rjk = sqrt(r2jk);
    q.rmjk = q.rjk * ANNP_CFLENGTH;
    if (!(q.rmb < p.rc_ang) || !(q.rmjk < p.rc_ang) || !(r2jk > 0.0)) return false;
    q.ct = (q.ja[0] * q.kb[0] + q.ja[1] * q.kb[1] + q.ja[2] * q.kb[2]) / (q.ra * q.rb);
    double sn, cs;
    sincos_0_pi(q.rmjk * p.por_ang, sn, cs);
    q.fcjk = 0.5 * (cs + 1.0); q.dfcjk = -0.5 * p.por_ang * sn;
    q.term_fc = L.fca[a] * L.fca[b] * q.fcjk;
    q.r2sum = q.rma * q.rma + q.rmb * q.rmb + q.rmjk * q.rmjk;
    return true;
}

// ---- descriptor pass ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64 * NIW_WAVES) void annp_niw_desc(const NiWideArgs p)
{
    __shared__ double s_rec[NIW_WAVES][8 * NIW_CAP];
    __shared__ int s_j[NIW_WAVES][NIW_CAP];
    ANNP_POISON();
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const int ii = blockIdx.x * NIW_WAVES + wave;
    if (ii >= p.inum) return;
    const NiwRec L = niw_records(s_rec[wave], s_j[wave]);
    const int i = p.ilist ? p.ilist[ii] : ii;
    const bool centre = !p.type || type_mapped(p.active, p.type[i]);
    int n = 0;
    if (centre) n = niw_filter(p, i, L, lane);
    if (n > NIW_CAP) {              // more than the records hold: reported, the atom is skipped (its row reads zero)
        if (lane == 0) atomicMax(p.errflag, n);
        n = 0;
    }
    double g = 0.0;
    if (lane < p.npsf) {            // radial function `lane` (ni:686-711; Rs is read by the reference and never used)
        const double eta = p.rad[3 * lane];
        for (int a = 0; a < n; a++) {
            const double rm = L.r[a] * ANNP_CFLENGTH;
            if (rm < p.rc_rad) g += exp(-eta * rm * rm) * L.fcr[a];
        }
    }
    const bool angular = lane >= p.npsf && lane < p.npsf + p.ntsf;
    double eta = 0.0, lam = 0.0, zeta = 1.0, coe = 0.0;
    if (angular) {
        const double *row = p.ang + 4 * (lane - p.npsf);
        eta = row[0]; lam = row[1]; zeta = row[2]; coe = row[3];
    }
    const int iz = niw_zeta_int(zeta);
    for (int a = 0; a + 1 < n; a++) {
        if (!(L.r[a] * ANNP_CFLENGTH < p.rc_ang)) continue;
        for (int b = a + 1; b < n; b++) {
            NiwPair q;
            if (!niw_pair(p, L, a, b, q)) continue;
            const double flag = 1.0 + lam * q.ct;
            if (angular && flag > 0.0) g += coe * niw_pow(flag, zeta, iz) * exp(-eta * q.r2sum) * q.term_fc;
        }
    }
    p.G[(size_t)ii * NIW_PITCH + lane] = g;
    if (lane == 0) p.ncount[ii] = n;
}

// ---- force pass --------------------------------------------------------------------------------------------------------------
template <bool VIRIAL>
__global__ __launch_bounds__(64 * NIW_WAVES) void annp_niw_force(const NiWideArgs p)
{
    __shared__ double s_rec[NIW_WAVES][8 * NIW_CAP];
    __shared__ double s_acc[NIW_WAVES][3 * NIW_CAP];
    __shared__ double s_c[NIW_WAVES][NIW_PITCH];
    __shared__ int s_j[NIW_WAVES][NIW_CAP];
    ANNP_POISON();
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const int ii = blockIdx.x * NIW_WAVES + wave;
    if (ii >= p.inum) return;
    const NiwRec L = niw_records(s_rec[wave], s_j[wave]);
    double *ax = s_acc[wave], *ay = ax + NIW_CAP, *az = ay + NIW_CAP, *crow = s_c[wave];
    const int i = p.ilist ? p.ilist[ii] : ii;
    if (p.type && !type_mapped(p.active, p.type[i])) return;
    const int n = niw_filter(p, i, L, lane);
    if (n == 0 || n > NIW_CAP) return;          // (above the capacity: the descriptor pass has reported it)
    crow[lane] = p.coef[(size_t)ii * NIW_PITCH + lane];
    wave_lds_sync();
    // radial part, lanes over the neighbours: sum_m c_m dG_m/dr, along -(xi - xj) / r (ni:699-708)
    for (int a = lane; a < n; a += ANNP_WAVE) {
        const double r = L.r[a], rm = r * ANNP_CFLENGTH;
        double S = 0.0;
        if (rm < p.rc_rad) {
            const double fc = L.fcr[a], dfc = L.dfcr[a];
            for (int m = 0; m < p.npsf; m++) {
                const double eta = p.rad[3 * m];
                S += crow[m] * exp(-eta * rm * rm) * (-fc * 2.0 * eta * rm + dfc);
            }
        }
        const double s = -S / r;
        ax[a] = s * L.dx[a]; ay[a] = s * L.dy[a]; az[a] = s * L.dz[a];
    }
    wave_lds_sync();
    // angular part, lane = function: three weighted sums over the functions per pair, then the pair's vectors once
    const bool angular = lane >= p.npsf && lane < p.npsf + p.ntsf;
    double eta = 0.0, lam = 0.0, zeta = 1.0, coe = 0.0, c = 0.0;
    if (angular) {
        const double *row = p.ang + 4 * (lane - p.npsf);
        eta = row[0]; lam = row[1]; zeta = row[2]; coe = row[3];
        c = crow[lane];
    }
    const int iz = niw_zeta_int(zeta);
    for (int a = 0; a + 1 < n; a++) {
        if (!(L.r[a] * ANNP_CFLENGTH < p.rc_ang)) continue;
        for (int b = a + 1; b < n; b++) {
            NiwPair q;
            if (!niw_pair(p, L, a, b, q)) continue;
            const double flag = 1.0 + lam * q.ct;
            double w1 = 0.0, w2 = 0.0, w3 = 0.0;
            if (angular && flag > 0.0) {
                const double term3 = coe * niw_pow(flag, zeta, iz) * exp(-eta * q.r2sum);       // term_cot term_exp (ni:748-756)
                w3 = c * term3;
                w2 = w3 * eta;
                w1 = w3 * lam * zeta / flag;
            }
            const double S1 = wave_sum(w1) * q.term_fc / ANNP_CFLENGTH;
            const double S2 = wave_sum(w2) * q.term_fc;
            const double S3 = wave_sum(w3);
            if (lane == 0) {
                const double fca = L.fca[a], fcb = L.fca[b], dfca = L.dfca[a], dfcb = L.dfca[b];
                const double B = q.ra * q.rb, c1 = q.ct / (q.ra * q.ra), c2 = q.ct / (q.rb * q.rb);
                // ni:737-738 multiply d r_jk by r_ik; the gradient-consistent form uses r_jk
                const double rjk_used = p.compat ? q.rmb : q.rmjk;
                double gj[3], gk[3];
#pragma unroll
                for (int d = 0; d < 3; d++) {
                    const double drj = -q.ja[d] / q.ra, drk = -q.kb[d] / q.rb, drjk = (q.kb[d] - q.ja[d]) / q.rjk;
                    const double dctj = -q.kb[d] / B + c1 * q.ja[d], dctk = -q.ja[d] / B + c2 * q.kb[d];
                    const double t2j = 2.0 * (q.rma * drj + rjk_used * drjk), t2k = 2.0 * (q.rmb * drk - rjk_used * drjk);
                    const double t3j = fcb * (dfca * drj * q.fcjk + fca * q.dfcjk * drjk);
                    const double t3k = fca * (dfcb * drk * q.fcjk - fcb * q.dfcjk * drjk);
                    gj[d] = S1 * dctj - S2 * t2j + S3 * t3j;
                    gk[d] = S1 * dctk - S2 * t2k + S3 * t3k;
                }
                ax[a] += gj[0]; ay[a] += gj[1]; az[a] += gj[2];
                ax[b] += gk[0]; ay[b] += gk[1]; az[b] += gk[2];
            }
        }
    }
    wave_lds_sync();
    // per-neighbour totals g = sum_n c_n dG_n/dx_j: F_j = -g CFFORCE, the centre takes the opposite sum (ni:186-203)
    double fi0 = 0.0, fi1 = 0.0, fi2 = 0.0;
    double v0 = 0.0, v1 = 0.0, v2 = 0.0, v3 = 0.0, v4 = 0.0, v5 = 0.0;
    for (int a = lane; a < n; a += ANNP_WAVE) {
        const double g0 = ax[a], g1 = ay[a], g2 = az[a];
        const int j = L.j[a];
        atomicAdd(&p.f[3 * (size_t)j], -g0 * ANNP_CFFORCE);
        atomicAdd(&p.f[3 * (size_t)j + 1], -g1 * ANNP_CFFORCE);
        atomicAdd(&p.f[3 * (size_t)j + 2], -g2 * ANNP_CFFORCE);
        fi0 += g0; fi1 += g1; fi2 += g2;
        if (VIRIAL) {           // the reference tallies the un-converted force (ni:190-198)
            const double d0 = L.dx[a], d1 = L.dy[a], d2 = L.dz[a];
            const double w0 = d0 * g0, w1 = d1 * g1, w2 = d2 * g2, w3 = d0 * g1, w4 = d0 * g2, w5 = d1 * g2;
            v0 += w0; v1 += w1; v2 += w2; v3 += w3; v4 += w4; v5 += w5;
            if (p.vatom) {
                double *vj = p.vatom + 6 * (size_t)j;
                atomicAdd(vj + 0, 0.5 * w0); atomicAdd(vj + 1, 0.5 * w1); atomicAdd(vj + 2, 0.5 * w2);
                atomicAdd(vj + 3, 0.5 * w3); atomicAdd(vj + 4, 0.5 * w4); atomicAdd(vj + 5, 0.5 * w5);
            }
        }
    }
    fi0 = wave_sum(fi0); fi1 = wave_sum(fi1); fi2 = wave_sum(fi2);
    if (lane == 0) {
        atomicAdd(&p.f[3 * (size_t)i], fi0 * ANNP_CFFORCE);
        atomicAdd(&p.f[3 * (size_t)i + 1], fi1 * ANNP_CFFORCE);
        atomicAdd(&p.f[3 * (size_t)i + 2], fi2 * ANNP_CFFORCE);
    }
    if (VIRIAL) {
        v0 = wave_sum(v0); v1 = wave_sum(v1); v2 = wave_sum(v2); v3 = wave_sum(v3); v4 = wave_sum(v4); v5 = wave_sum(v5);
        if (lane == 0) {
            if (p.vatom) {
                double *vi = p.vatom + 6 * (size_t)i;
                atomicAdd(vi + 0, 0.5 * v0); atomicAdd(vi + 1, 0.5 * v1); atomicAdd(vi + 2, 0.5 * v2);
                atomicAdd(vi + 3, 0.5 * v3); atomicAdd(vi + 4, 0.5 * v4); atomicAdd(vi + 5, 0.5 * v5);
            }
            if (p.virial) {
                double *vr = virial_row(p.virial);
                atomicAdd(&vr[0], v0); atomicAdd(&vr[1], v1); atomicAdd(&vr[2], v2);
                atomicAdd(&vr[3], v3); atomicAdd(&vr[4], v4); atomicAdd(&vr[5], v5);
            }
        }
    }
}

// ---- network pass ------------------------------------------------------------------------------------------------------------
// Forward and reverse sweep of ni:769-867 for NIW_MA atoms at a time, lane = node.  A layer's inputs stand in LDS (one row per atom)
// and are read as broadcasts; its weights come from the image, one coalesced 512-byte row per input (forward: the transpose,
// backward: the matrix itself), each used for the NIW_MA atoms.  One launch per element: atoms of other elements are left alone.
__global__ __launch_bounds__(64 * NIW_WAVES) void annp_mlp_wide(const MlpWideArgs p)
{
    __shared__ double s_h[NIW_WAVES][NIW_MA][64];
    __shared__ double s_e[NIW_WAVES];
    ANNP_POISON();
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    double (*h)[64] = s_h[wave];
    ActParam ap[MLP_MAXL];
#pragma unroll
    for (int l = 0; l < MLP_MAXL; l++) ap[l] = act_param(p.act[l], p.act_plain);
    const double *bias = p.img + (size_t)MLP_MAXL * NIW_LAYER;
    const double nsub = p.nsub[lane], nden = p.nden[lane], cmul = p.cmul[lane];
    const int nl = uniform(p.nl), nnod = uniform(p.nnod), nsf = uniform(p.nsf);
    double e_wave = 0.0;
    const int ngroups = (p.inum + NIW_MA - 1) / NIW_MA;
    for (int grp = blockIdx.x * NIW_WAVES + wave; grp < ngroups; grp += gridDim.x * NIW_WAVES) {
        bool val[NIW_MA];
        bool any = false;
#pragma unroll
        for (int a = 0; a < NIW_MA; a++) {
            const int ia = grp * NIW_MA + a;
            val[a] = ia < p.inum;
            if (val[a] && p.type) {
                const int t = p.type[p.ilist ? p.ilist[ia] : ia];
                val[a] = type_mapped(p.active, t) && p.map[t] == p.elem;
            }
            any = any || val[a];
        }
        if (!any) continue;
        wave_lds_sync();            // the trip before is done with the rows
#pragma unroll
        for (int a = 0; a < NIW_MA; a++)
            h[a][lane] = (val[a] && lane < nsf) ? (p.G[(size_t)(grp * NIW_MA + a) * NIW_PITCH + lane] - nsub) * nden : 0.0;
        wave_lds_sync();
        double D[MLP_MAXL][NIW_MA];
        int din = nsf;
#pragma unroll
        for (int l = 0; l < MLP_MAXL; l++) {
            if (l >= nl) continue;
            const int dout = l == nl - 1 ? 1 : nnod;
            const double *wt = p.img + (size_t)l * NIW_LAYER + 64 * 64;
            double acc[NIW_MA];
            const double b = bias[64 * l + lane];
#pragma unroll
            for (int a = 0; a < NIW_MA; a++) acc[a] = b;
            for (int k = 0; k < din; k++) {
                const double w = wt[64 * k + lane];
#pragma unroll
                for (int a = 0; a < NIW_MA; a++) acc[a] = fma(w, h[a][k], acc[a]);
            }
            wave_lds_sync();        // every lane has read the layer's inputs: the outputs take their place
#pragma unroll
            for (int a = 0; a < NIW_MA; a++) {
                double hh = 0.0, dd = 0.0;
                if (lane < dout) activation(ap[l], acc[a], hh, dd);
                D[l][a] = dd;
                h[a][lane] = hh;
            }
            wave_lds_sync();
            din = dout;
        }
        // energy: the network's output (ni:858-860)
#pragma unroll
        for (int a = 0; a < NIW_MA; a++) {
            if (val[a] && lane == 0) {
                const double e = h[a][0];
                e_wave += e;
                if (p.eatom) {
                    const int ia = grp * NIW_MA + a;
                    p.eatom[p.ilist ? p.ilist[ia] : ia] += e;
                }
            }
        }
        // reverse sweep: delta of the output layer is its activation's derivative; dE/dGhat = W_0^T delta_0
        double dl[NIW_MA];
#pragma unroll
        for (int a = 0; a < NIW_MA; a++) dl[a] = 0.0;
#pragma unroll
        for (int l = MLP_MAXL - 1; l >= 0; l--) {
            if (l >= nl) continue;
            const int dout = l == nl - 1 ? 1 : nnod;
            if (l == nl - 1) {
#pragma unroll
                for (int a = 0; a < NIW_MA; a++) dl[a] = D[l][a];         // (zero beyond lane 0)
            }
            wave_lds_sync();
#pragma unroll
            for (int a = 0; a < NIW_MA; a++) h[a][lane] = dl[a];
            wave_lds_sync();
            const double *w = p.img + (size_t)l * NIW_LAYER;
            double s[NIW_MA];
#pragma unroll
            for (int a = 0; a < NIW_MA; a++) s[a] = 0.0;
            for (int r = 0; r < dout; r++) {
                const double wv = w[64 * r + lane];
#pragma unroll
                for (int a = 0; a < NIW_MA; a++) s[a] = fma(wv, h[a][r], s[a]);
            }
            if (l > 0) {
#pragma unroll
                for (int a = 0; a < NIW_MA; a++) dl[a] = s[a] * D[l - 1][a];
            } else {
#pragma unroll
                for (int a = 0; a < NIW_MA; a++)
                    if (val[a]) p.coef[(size_t)(grp * NIW_MA + a) * NIW_PITCH + lane] = cmul * s[a];
            }
        }
    }
    // one atomic per workgroup on the energy word
    if (p.eng) {
        if (lane == 0) s_e[wave] = e_wave;
        __syncthreads();
        if (threadIdx.x == 0) {
            double e = 0.0;
#pragma unroll
            for (int w = 0; w < NIW_WAVES; w++) e += s_e[w];
            if (e != 0.0) atomicAdd(p.eng, e);
        }
    }
}

inline int niw_blocks(int inum) { return (inum + NIW_WAVES - 1) / NIW_WAVES; }
inline int niw_mlp_blocks(int inum)
{
    const int groups = (inum + NIW_MA - 1) / NIW_MA;
    const int b = (groups + NIW_WAVES - 1) / NIW_WAVES;
    return b < 1 ? 1 : (b > NIW_MAX_BLOCKS ? NIW_MAX_BLOCKS : b);
}

}  // namespace annp
