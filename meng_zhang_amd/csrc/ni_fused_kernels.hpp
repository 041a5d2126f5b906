// ni_fused_kernels.hpp -- the Behler G2/G4 evaluation of one atom group in ONE kernel: records, descriptor, network, force
// (ANNP_HIP_NI_EVAL=fused; the default route stays the three passes of ni_kernels.hpp / mlp_kernels.hpp).
//
// What the three launches move through memory only because they are three launches: the descriptor rows G (written, read by the
// network), the coefficient rows (written by the network, read by the force pass), the compacted neighbour rows and the pair lists
// (written by the descriptor pass, read by the force pass), and the ~18 in-range neighbours of every atom gathered a second time.
// Here a wave keeps all of that in its LDS: same wave shape as the passes (four atoms per wave, a 16-lane group per atom, a wave walks
// a run of NI_RUN groups and sends their forces through one wave-private table), and per group
//   1. stage      ni_stage<true>: filter the four list rows, records at their true place (the force needs the direction of a
//                 neighbour that is only inside the radial cutoff), then ni_prepass<true> over ALL trips into an LDS pair list;
//   2. descriptor G2 over the records, G4 over the pair list; the 16 lane partials of every sum meet in the group's last lane
//                 (DPP row shifts: the records are live, there is no LDS to spare for a transposed reduction);
//   3. network    on the vector unit inside the atom's 16-lane group: lane l owns nodes l and l + 16, the previous layer is read
//                 from the atom's LDS row as broadcasts, a layer's outputs replace its inputs IN that row (every lane has read the
//                 whole row before any lane writes: one row of 34 doubles per atom is the network's whole LDS).  The weights are
//                 NOT in LDS: an image of them would be the third resident workgroup (see ni_fused_lds_block); they are read from
//                 a global image laid out so that the two nodes of a lane are one 16-byte load and a group's loads one 256-byte
//                 line, the same line for all four groups of the wave and every wave of the CU (14 KB for the shipped network);
//   4. force      ni_records (radial part into the accumulators, table slots), then the force visit over the same records and the
//                 same pair list, forces into the run's table, flushed with global atomics at the end of the run;
//   5. energy     eatom per atom, the run's total with one atomic per wave.
// G rows, ncount and the in-cutoff maximum are still written (the getters of annp_hip.h behave as on the passes route); nothing
// else goes to memory.  A group that outgrows its records is queued and taken by the FIX instantiation, as in the passes.
// No workgroup ever waits for another one: no flag is polled, there is no grid-wide barrier.
#pragma once
#include "mlp_kernels.hpp"
#include "ni_kernels.hpp"

namespace annp {

// ---- the network image (global memory) ----------------------------------------------------------------------------------------
// "Pair-interleaved": element (row r, lane l, u) at (r * 16 + l) * 2 + u belongs to the lane's node / feature l + 16 u.
//   f0   [nsf ][32]   W_0[own node][k]         features k in VISIT order (radial, then angular as the kernels visit them)
//   fh   [nlw-2][nnod][32]   W_l[own node][m]  hidden layers l = 1 .. nlw-2, forward
//   wo   [32]         W_out[own node]
//   bias [nlw-1][32]  b_l[own node], then b_out (one double, one of padding)
//   bk   [nlw-2][nnod][32]   W_l[n][own node m]  the same hidden layers, backward
//   b0   [nnod][32]   W_0[i][own feature k]
//   norm [3][32]      nmul | nsub | nden of the own feature (visit order; 0 beyond nsf)
// Everything beyond nsf / nnod is zero.
struct NiNet { int f0, fh, wo, bias, bk, b0, norm, total; };
__host__ __device__ inline NiNet ni_net_layout(int nsf, int nnod, int nlw)
{
    NiNet t;
    int o = 0;
    t.f0 = o; o += nsf * 32;
    t.fh = o; o += (nlw - 2) * nnod * 32;
    t.wo = o; o += 32;
    t.bias = o; o += (nlw - 1) * 32 + 2;
    t.bk = o; o += (nlw - 2) * nnod * 32;
    t.b0 = o; o += nnod * 32;
    t.norm = o; o += 3 * 32;
    t.total = o;
    return t;
}

// Host: W[l] row-major [d_{l+1}][d_l] with layer 0 in the FILE's feature order, B[l]; vis[v] = file index of visit position v;
// norm = nmul | nsub | nden, ANNP_GPAD each, file order.
inline void ni_net_build(double *img, const double *const *W, const double *const *B, const int *vis, const double *norm, int nsf, int nnod, int nlw)
{
    const NiNet t = ni_net_layout(nsf, nnod, nlw);
    for (int o = 0; o < t.total; o++) img[o] = 0.0;
    auto at = [](int r, int own) { return (r * 16 + (own & 15)) * 2 + (own >> 4); };
    for (int n = 0; n < nnod; n++)
        for (int v = 0; v < nsf; v++) {
            img[t.f0 + at(v, n)] = W[0][(size_t)n * nsf + vis[v]];
            img[t.b0 + at(n, v)] = W[0][(size_t)n * nsf + vis[v]];
        }
    for (int l = 1; l <= nlw - 2; l++)
        for (int n = 0; n < nnod; n++)
            for (int m = 0; m < nnod; m++) {
                img[t.fh + (l - 1) * nnod * 32 + at(m, n)] = W[l][(size_t)n * nnod + m];
                img[t.bk + (l - 1) * nnod * 32 + at(n, m)] = W[l][(size_t)n * nnod + m];
            }
    for (int n = 0; n < nnod; n++) img[t.wo + at(0, n)] = W[nlw - 1][n];
    for (int l = 0; l <= nlw - 2; l++)
        for (int n = 0; n < nnod; n++) img[t.bias + l * 32 + at(0, n)] = B[l][n];
    img[t.bias + (nlw - 1) * 32] = B[nlw - 1][0];
    for (int v = 0; v < nsf; v++)
        for (int a = 0; a < 3; a++) img[t.norm + a * 32 + at(0, v)] = norm[a * ANNP_GPAD + vis[v]];
}

struct NiFusedArgs {
    NiArgs n;                   // as the passes (coef, nbr, pairs, npair, skip_above unused)
    const double *net;          // ni_net_build
    int nnod, nlw;              // nodes per hidden layer (<= 32), weight layers (2 .. MLP_MAXL)
    int act[MLP_MAXL];          // activation flags (ni: 3 and 4 are plain tanh, as MlpArgs::act_plain)
    double *eatom, *eng;        // nullable
    int *nmax_word;             // raised to the largest in-range count of the evaluated groups (what annp_max_int makes of ncount on the passes route)
};

// ---- LDS of one wave -----------------------------------------------------------------------------------------------------------
// ten record arrays (dx dy dz r 1/r fc fc' | three force accumulators) of 4 cap + 2 doubles, the atoms' network rows (which end as
// their coefficient rows), the run's force table, the integer side of the records, and the atoms' in-range pair lists -- all
// cap (cap - 1) / 2 candidates could be in range.  At capacity 20: 13 504 bytes.
__host__ __device__ constexpr int ni_fused_plist(int cap) { return (cap * (cap - 1) / 2 + 7) / 8 * 8; }
__host__ __device__ constexpr size_t ni_fused_lds_per_wave(int cap)
{
    const size_t R = (size_t)NI_GA * cap + 2;
    const size_t b = R * 10 * 8 + (size_t)NI_GA * NI_CSTRIDE * 8 + (size_t)NI_TSLOTS * (3 * 8 + 4) + R * 8 + 2 * NI_GA * 4 + (size_t)NI_GA * ni_fused_plist(cap) * 2 +
                     NI_GA * 4 + NI_GA * 8;       // + the atoms' pair counts and the run's energy, one slot per group of lanes
    return (b + 15) / 16 * 16;
}
// (the table-driven instantiation keeps the sorted function table in front of the waves, as the passes do)
__host__ __device__ constexpr size_t ni_fused_lds_block(int cap, bool generic)
{
    return (generic ? (size_t)NI_TABLE_DOUBLES * 8 : 0) + ni_fused_lds_per_wave(cap) * ANNP_WAVES_PER_BLOCK;
}
// three workgroups per CU in the steady state (160 KB / 3); a 14 KB weight image in LDS would make it two
static_assert(ni_fused_lds_block(NI_CAP_FIXED, false) <= 53 * 1024, "annp_ni_fused: three workgroups per CU at record capacity 20");

inline int ni_fused_max_cap(bool generic)
{
    int cap = 8;
    while (cap + 8 <= 248 && ni_fused_lds_block(cap + 8, generic) <= 160 * 1024) cap += 8;     // (a pair entry holds two 8-bit record slots)
    return cap;
}

__device__ __forceinline__ NiLds ni_fused_carve(unsigned char *wbase, int cap, int plist)
{
    NiLds L;
    const int R = NI_GA * cap + 2;
    double *d = reinterpret_cast<double *>(wbase);
    L.dx = d; L.dy = L.dx + R; L.dz = L.dy + R; L.r = L.dz + R; L.rinv = L.r + R; L.fc = L.rinv + R; L.dfc = L.fc + R;
    L.a0 = L.dfc + R; L.a1 = L.a0 + R; L.a2 = L.a1 + R;
    L.coef = L.a2 + R; L.tacc = L.coef + NI_GA * NI_CSTRIDE;
    L.j = reinterpret_cast<int *>(L.tacc + 3 * NI_TSLOTS);
    L.sl = L.j + R; L.ci = L.sl + R; L.cs = L.ci + NI_GA; L.tkey = L.cs + NI_GA;
    L.pl = reinterpret_cast<unsigned short *>(L.tkey + NI_TSLOTS);
    (void)plist;
    return L;
}

// tanh_fast (mlp_kernels.hpp: same operations, same results) with the polynomial's coefficients from constant memory through the scalar
// unit where they are used -- they are the expm1 coefficients of exp_neg_s.  As 64-bit literals the compiler builds them once before
// the run, keeps them across the pair loops and spills what the pair loops need.
__device__ __forceinline__ double tanh_fast_s(double y)
{
    const annp_cptr T = mtab_scalar();
    const double x = fmax(-2.0 * fabs(y), -80.0);
    const double kf = rint(x * T[22]);
    double r = fma(-kf, T[23], x);
    r = fma(-kf, T[24], r);
    double q = T[25];
#pragma unroll
    for (int k = 26; k < ANNP_MTAB; k++) q = fma_vvs(q, r, T[k]);
    q = fma(q, r, 0.5);
    q = fma(q, r, 1.0);
    q = q * r;
    const int k = (int)kf;
    const double em1 = (k == 0) ? q : __builtin_ldexp(1.0 + q, k) - 1.0;
    const double d = 2.0 + em1;
    double rc = __builtin_amdgcn_rcp(d);
    rc = fma(rc, fma(-d, rc, 1.0), rc);
    rc = fma(rc, fma(-d, rc, 1.0), rc);
    double t = -em1 * rc;
    t = fma(fma(-d, t, -em1), rc, t);
    return copysign(t, y);
}
// activation of mlp_kernels.hpp for a layer's flag (ni: 3 and 4 are plain tanh); the flag is made opaque so that the five numbers it
// selects are formed here, not before the run
__device__ __forceinline__ void ni_fused_act(int flag, double a, double &h, double &dh)
{
    asm volatile("" : "+s"(flag));
    const ActParam q = act_param(flag, 1);
    const double t = tanh_fast_s(q.s * a);
    h = fma(q.A, t, fma(q.C, a, q.D));
    dh = fma(q.P, fma(-t, t, 1.0), q.C);
}

// z0, z1 += sum_k W[k][own nodes] row[k]: the weights of a lane's two nodes are one 16-byte load, the inputs LDS broadcasts
__device__ __forceinline__ void ni_fused_matvec(const double *W, const double *row, int nin, int l, double &z0, double &z1)
{
    const double2 *w2 = reinterpret_cast<const double2 *>(W) + l;
#pragma unroll 4
    for (int k = 0; k < nin; k++) {
        const double2 w = w2[k * 16];
        const double x = row[k];
        z0 = fma(w.x, x, z0); z1 = fma(w.y, x, z1);
    }
}

// a layer's outputs take the place of its inputs: every lane has read the row (the values are in registers) before any lane writes
__device__ __forceinline__ void ni_fused_row_put(double *row, int l, double v0, double v1)
{
    wave_lds_sync();
    row[l] = v0; row[l + NI_GL] = v1;
    wave_lds_sync();
}

// ---------------------------------------------------------------------------------------------------------------------------------
// FIX: the fix-up instantiation (its waves walk the queue of groups that outgrew the main launch's records; 2 waves per SIMD)
// CAP > 0: the record capacity is compiled in (p.n_cap equals it): record arrays at constant offsets, as in the force pass
template <int NP, int NT, int NL, int NE, int NZ, unsigned ZP, unsigned EM, bool VIRIAL, bool FIX, int CAP = 0>
// (the virial instantiations get 2 waves per SIMD: at 3 the compiler spills 2-4 vector registers to scratch in them, wherever the tally
// stands -- inside the force sweep or in a sweep of its own; the steady state of an MD run, without the tally, keeps 3)
__global__ __launch_bounds__(256, (FIX || VIRIAL) ? 2 : 3) void annp_ni_fused(NiFusedArgs q)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    ANNP_POISON();
    const NiArgs &p = q.n;
    const int lane0 = lane_id();
    const int wave = uniform(threadIdx.x >> 6);
    const int run = uniform((FIX ? (int)blockIdx.x : xcd_block()) * ANNP_WAVES_PER_BLOCK + wave);
    const int nslots = FIX ? min(*p.ovf_count, p.ovf_cap) : 0;       // fix-up launch: a small grid whose waves walk the queue
    const int nwaves = (int)gridDim.x * ANNP_WAVES_PER_BLOCK;
    const int nsf = p.npsf + p.ntsf;
    const int cap = CAP > 0 ? CAP : p.n_cap;
    const int plist = ni_fused_plist(cap);
    NiTab tab = ni_tab(p.sym, p.isym, p.npsf, p.ntsf, nullptr);
    const double *srad = tab.rad;
    ni_tables_fill<NL, NE, NZ>(reinterpret_cast<double *>(lds_raw), p, tab, lane0);
    unsigned char *wbase = lds_raw + (NL == 0 ? NI_TABLE_DOUBLES * 8 : 0) + (size_t)wave * ni_fused_lds_per_wave(cap);
    const NiLds L = ni_fused_carve(wbase, cap, plist);
    for (int sl = lane0; sl < NI_TSLOTS; sl += 64) { L.tkey[sl] = -1; L.tacc[3 * sl] = 0.0; L.tacc[3 * sl + 1] = 0.0; L.tacc[3 * sl + 2] = 0.0; }
    wave_lds_sync();
    // what would otherwise live in vector registers across the pair loops (the force visit has none to spare): the atoms' pair counts
    // between the two visits, and the energies of the run's atoms, one sum per group of lanes
    int *pcnt = reinterpret_cast<int *>(L.pl + NI_GA * plist);
    double *esum = reinterpret_cast<double *>(pcnt + NI_GA);
    if (lane0 < NI_GA) esum[lane0] = 0.0;
    const NiNet net = ni_net_layout(nsf, q.nnod, q.nlw);
    int nmax_run = 0;           // largest in-range count of the groups this wave evaluated
#pragma unroll 1
    for (int gk = 0;; gk++) {
    int ii0;
    if (!FIX) {
        if (gk >= NI_RUN) break;
        ii0 = uniform((run * NI_RUN + gk) * NI_GA);
    } else {
        const int slot = run + gk * nwaves;
        if (slot >= nslots) break;
        ii0 = uniform(p.ovf_list[slot]);
    }
    if (ii0 >= p.inum) break;
    ni_forget_lds();            // nothing read from LDS is carried from one group to the next in registers
    // (the lane number is opaque per group, as in the passes: per-lane LDS addresses are formed where they are used instead of being
    // computed before the run, kept live across the pair loops and spilled)
    int lane = lane0;
    asm volatile("" : "+v"(lane));
    const int g = lane >> 4, l = lane & 15;

    // ---- 1. stage ------------------------------------------------------------------------------------------------------------
    const NiHead head = ni_stage_head(p, ii0, lane);
    int nl;
    const int nmax = ni_stage<true>(p, head, L, cap, lane, nl);
    const int ncl = __shfl(nl, NI_GL * (lane & (NI_GA - 1)), 64);     // count of atom (lane & 3), for lanes 0..3
    if (p.ncount && lane < NI_GA && ii0 + lane < p.inum) p.ncount[ii0 + lane] = nmax > cap ? 0 : ncl;
    if (nmax > cap) {           // more than these records hold: the fix-up launch's (its records hold a whole list row), else an error
        if (lane == 0) {
            bool queued = false;
            if (!FIX && p.ovf_list) {
                const int qs = atomicAdd(p.ovf_count, 1);
                queued = qs < p.ovf_cap;
                if (queued) p.ovf_list[qs] = ii0;
            }
            if (!queued) atomicMax(p.errflag, nmax);
        }
        for (int idx = lane; idx < NI_GA * ANNP_GPAD; idx += 64)
            if (ii0 + idx / ANNP_GPAD < p.inum) p.G[(size_t)ii0 * ANNP_GPAD + idx] = 0.0;
        wave_lds_sync();
        continue;
    }
    nmax_run = max(nmax_run, nmax);
    wave_lds_sync();
    const int sbase = g * cap;
    double *row = L.coef + g * NI_CSTRIDE;          // the atom's network row: G, Ghat, layers, deltas, at last its coefficients
    const int npl = nl * (nl - 1) / 2;
    const int trips = (nmax * (nmax - 1) / 2 + NI_GL - 1) / NI_GL;
    NiWalk walk = ni_walk_init(l, nl);
    const int cnt = ni_prepass<true>(L, p, walk, g, l, sbase, cap, npl, 0, trips, plist);      // the atom's in-range pairs, for both visits
    if (l == 0) pcnt[g] = cnt;
    wave_lds_sync();

    // ---- 2. descriptor (the arithmetic of annp_ni_desc) ----------------------------------------------------------------------
    {
        double gr[NP], ga[NT];
#pragma unroll
        for (int m = 0; m < NP; m++) gr[m] = 0.0;
#pragma unroll
        for (int m = 0; m < NT; m++) ga[m] = 0.0;      // indexed by visit position
        // G2 (ni:686-711): lane l of the group owns neighbours l, l+16, ...; a lane with nothing to add reads the dummy record
        const bool same_rc = p.rc_rad == p.rc_ang;
        for (int a = l; a < nmax; a += 2 * NI_GL) {
            const bool t0 = a < nl, t1 = a + NI_GL < nl;
            const int s0 = t0 ? sbase + a : NI_GA * cap, s1 = t1 ? sbase + a + NI_GL : NI_GA * cap;
            const double m0 = fmin(L.r[s0] * ANNP_CFLENGTH, p.rc_rad), m1 = fmin(L.r[s1] * ANNP_CFLENGTH, p.rc_rad);
            double f0, f1;
            if (same_rc) { f0 = L.fc[s0]; f1 = L.fc[s1]; }
            else {
                double sn0, cs0, sn1, cs1;
                sincos_0_pi_s2(p.por_rad * m0, p.por_rad * m1, sn0, cs0, sn1, cs1);
                f0 = 0.5 * (cs0 + 1.0); f1 = 0.5 * (cs1 + 1.0);
            }
            const bool in0 = t0 && L.r[s0] * ANNP_CFLENGTH < p.rc_rad, in1 = t1 && L.r[s1] * ANNP_CFLENGTH < p.rc_rad;    // ni:693
            if (!in0) f0 = 0.0;
            if (!in1) f1 = 0.0;
            double e0, e1;
            exp_neg_s2(-srad[0] * m0 * m0, -srad[0] * m1 * m1, e0, e1);
#pragma unroll
            for (int m = 0; m < NP; m++)
                if (m < p.npsf) {
                    const int km = NL > 0 ? NI_BYTE(EM, m & 3) : (int)((p.rad_em >> (8 * m)) & 255ull);
                    const double v0 = (km > 0 ? ni_powi(e0, km) : exp_neg_s(-srad[3 * m] * m0 * m0)) * f0;
                    const double v1 = (km > 0 ? ni_powi(e1, km) : exp_neg_s(-srad[3 * m] * m1 * m1)) * f1;
                    gr[m] += in0 ? v0 : 0.0;
                    gr[m] += in1 ? v1 : 0.0;
                }
        }
        // G4 (ni:713-767) over the pair list
        const int cmax = max(max(__builtin_amdgcn_readlane(cnt, 0), __builtin_amdgcn_readlane(cnt, 16)),
                             max(__builtin_amdgcn_readlane(cnt, 32), __builtin_amdgcn_readlane(cnt, 48)));
        for (int t2 = 0; t2 * NI_GL < cmax; t2++) {
            const int idx = t2 * NI_GL + l;
            const bool live = idx < cnt;
            const int v = live ? L.pl[g * plist + idx] : 0;
            const NiPairS pr = ni_pair(L, p, live ? sbase + (v & 255) : NI_GA * cap, live ? sbase + (v >> 8) : NI_GA * cap + 1);
            const double r2sum = pr.rjm * pr.rjm + pr.rkm * pr.rkm + pr.rgm * pr.rgm;
            const double tfc = pr.tfc;                                  // idle lanes add zeros
            ni_forget_lds();
            if constexpr (NL > 0) ni_desc_cart<NL, NE, NZ, ZP, EM, NT>(p, pr.ct, r2sum, tfc, ga);
            else
                ni_visit_functions<NT, false>(tab, p.ntsf, pr.ct, r2sum,
                                              [&](int pos, double val, double) { ga[pos] = fma(val, tfc, ga[pos]); });
        }
        // the 16 lane partials of every sum meet in the group's last lane, which leaves them in the atom's row (visit order)
#pragma unroll
        for (int m = 0; m < NP; m++) {
            const double s = row16_sum_to_last(gr[m]);
            if (l == NI_GL - 1 && m < p.npsf) row[m] = s;
        }
#pragma unroll
        for (int m = 0; m < NT; m++) {
            const double s = row16_sum_to_last(ga[m]);
            if (l == NI_GL - 1 && m < p.ntsf) row[p.npsf + m] = s;
        }
    }
    wave_lds_sync();

    // ---- 3. network (the arithmetic of annp_mlp_mfma with act_plain = 1, energy_raw = 1) ---------------------------------------
    {
        const int i = L.ci[g];      // the centre, -1: none (the last group of the list)
        const int k0 = l, k1 = l + NI_GL;       // this lane's features (visit order), then its nodes
        const double raw0 = k0 < nsf ? row[k0] : 0.0, raw1 = k1 < nsf ? row[k1] : 0.0;
        if (i >= 0) {           // the descriptor row, in the file's order, zeros behind it (annp_hip_last_descriptors)
            double *Gi = p.G + (size_t)(ii0 + g) * ANNP_GPAD;
            const int f0 = k0 < p.npsf ? k0 : (k0 < nsf ? p.npsf + tab.perm[k0 - p.npsf] : k0);
            const int f1 = k1 < p.npsf ? k1 : (k1 < nsf ? p.npsf + tab.perm[k1 - p.npsf] : k1);
            Gi[f0] = raw0; Gi[f1] = raw1;
        }
        const double2 nm = reinterpret_cast<const double2 *>(q.net + net.norm)[l], ns = reinterpret_cast<const double2 *>(q.net + net.norm + 32)[l],
                      nd = reinterpret_cast<const double2 *>(q.net + net.norm + 64)[l];
        ni_fused_row_put(row, l, fma(raw0, nm.x, -ns.x) * nd.x, fma(raw1, nm.y, -ns.y) * nd.y);       // Ghat (0 beyond nsf: nden = 0 there)
        const bool n0 = k0 < q.nnod, n1 = k1 < q.nnod;
        double dh[MLP_MAXL - 1][2];             // act'(z) of the hidden layers, this lane's nodes
        double h0 = 0.0, h1 = 0.0;
#pragma unroll
        for (int ly = 0; ly < MLP_MAXL - 1; ly++) {
            dh[ly][0] = 0.0; dh[ly][1] = 0.0;
            if (ly < q.nlw - 1) {
                const double2 b = reinterpret_cast<const double2 *>(q.net + net.bias + ly * 32)[l];
                double z0 = b.x, z1 = b.y;
                if (ly == 0) ni_fused_matvec(q.net + net.f0, row, nsf, l, z0, z1);
                else ni_fused_matvec(q.net + net.fh + (ly - 1) * q.nnod * 32, row, q.nnod, l, z0, z1);
                double a0, a1, d0, d1;
                ni_fused_act(q.act[ly], z0, a0, d0); ni_fused_act(q.act[ly], z1, a1, d1);
                h0 = n0 ? a0 : 0.0; h1 = n1 ? a1 : 0.0;           // (a node the network does not have: act(0) need not be 0)
                dh[ly][0] = n0 ? d0 : 0.0; dh[ly][1] = n1 ? d1 : 0.0;
                ni_fused_row_put(row, l, h0, h1);
            }
        }
        const double2 wo = reinterpret_cast<const double2 *>(q.net + net.wo)[l];
        double zo = fma(wo.x, h0, wo.y * h1);
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) zo += __shfl_xor(zo, off, 64);
        zo += q.net[net.bias + (q.nlw - 1) * 32];
        double out, dout;
        int oflag = q.act[0];                   // (selected, not indexed: the flags are kernel arguments)
#pragma unroll
        for (int ly = 1; ly < MLP_MAXL; ly++) if (ly == q.nlw - 1) oflag = q.act[ly];
        ni_fused_act(oflag, zo, out, dout);
        if (l == 0 && i >= 0) {                 // ni:858-860: E_i is the network's output
            esum[g] += out;
            if (q.eatom) q.eatom[i] += out;
        }
        // backward: delta of the last hidden layer, through the hidden layers, then dE/dGhat_k / (sf_max - sf_min)_k
        double d0 = 0.0, d1 = 0.0;
#pragma unroll
        for (int ly = 0; ly < MLP_MAXL - 1; ly++)
            if (ly == q.nlw - 2) { d0 = wo.x * dout * dh[ly][0]; d1 = wo.y * dout * dh[ly][1]; }
#pragma unroll
        for (int ly = MLP_MAXL - 2; ly >= 1; ly--)
            if (ly <= q.nlw - 2) {
                ni_fused_row_put(row, l, d0, d1);
                double s0 = 0.0, s1 = 0.0;
                ni_fused_matvec(q.net + net.bk + (ly - 1) * q.nnod * 32, row, q.nnod, l, s0, s1);
                d0 = s0 * dh[ly - 1][0]; d1 = s1 * dh[ly - 1][1];
            }
        ni_fused_row_put(row, l, d0, d1);
        double c0 = 0.0, c1 = 0.0;
        ni_fused_matvec(q.net + net.b0, row, q.nnod, l, c0, c1);
        ni_fused_row_put(row, l, c0 * nd.x, c1 * nd.y);          // the coefficient row: radial, then angular in visit order
    }

    // ---- 4. force (the arithmetic of annp_ni_force) ---------------------------------------------------------------------------
    {   // table slots, and the records again with the radial part in their accumulators (ni_records)
        const bool t0 = l < nl, t1 = l + NI_GL < nl;
        const int s0 = t0 ? sbase + l : NI_GA * cap, s1 = t1 ? sbase + l + NI_GL : NI_GA * cap;
        const int jj0 = t0 ? L.j[s0] : 0, jj1 = t1 ? L.j[s1] : 0;
        const double dx0 = L.dx[s0], dy0 = L.dy[s0], dz0 = L.dz[s0], dx1 = L.dx[s1], dy1 = L.dy[s1], dz1 = L.dz[s1];
        const int hi = L.ci[lane & (NI_GA - 1)];
        int sl0, sl1, sc;
        ni_table_claim3(L.tkey, t0, jj0, t1, jj1, lane < NI_GA && hi >= 0, hi, sl0, sl1, sc);
        if (lane < NI_GA) L.cs[lane] = sc;
        if (nmax > NI_GL)
            ni_records<NP, NL, EM, 2>(p, L, srad, row, {sbase + l, sbase + l + NI_GL}, {t0, t1}, {dx0, dx1}, {dy0, dy1}, {dz0, dz1}, {jj0, jj1}, {sl0, sl1});
        else
            ni_records<NP, NL, EM, 1>(p, L, srad, row, {sbase + l}, {t0}, {dx0}, {dy0}, {dz0}, {jj0}, {sl0});
        for (int a = l + 2 * NI_GL; a < nmax; a += NI_GL) {         // rows longer than two entries per lane (dense systems, the fix-up launch)
            const bool there = a < nl;
            const int s = there ? sbase + a : NI_GA * cap;
            const int j = there ? L.j[s] : 0;
            const double ex = L.dx[s], ey = L.dy[s], ez = L.dz[s];
            int slot, u1, u2;
            ni_table_claim3(L.tkey, there, j, false, 0, false, 0, slot, u1, u2);
            ni_records<NP, NL, EM, 1>(p, L, srad, row, {sbase + min(a, cap - 1)}, {there}, {ex}, {ey}, {ez}, {j}, {slot});
        }
    }
    wave_lds_sync();
    const double *cw = row + p.npsf;        // angular weights of this lane's atom, visit order
    const int cntf = pcnt[g];
    const int cmaxf = max(max(pcnt[0], pcnt[1]), max(pcnt[2], pcnt[3]));
    for (int t2 = 0; t2 * NI_GL < uniform(cmaxf); t2++) {
        const int idx = t2 * NI_GL + l;
        const bool lv = idx < cntf;
        const int pv = lv ? L.pl[g * plist + idx] : 0;
        const int sa = lv ? sbase + (pv & 255) : NI_GA * cap, sb = lv ? sbase + (pv >> 8) : NI_GA * cap + 1;
        const NiPairS pr = ni_pair(L, p, sa, sb);
        const double r2sum = pr.rjm * pr.rjm + pr.rkm * pr.rkm + pr.rgm * pr.rgm;
        if (pr.ok) {
            // A1 = sum c term1 CFLENGTH, A2 = sum c term2, A3 = sum c term3   (ni:752-754)
            double A1 = 0.0, A2 = 0.0, A3 = 0.0;
            ni_forget_lds();
            if constexpr (NL > 0) ni_force_cart<NL, NE, NZ, ZP, EM>(p, cw, pr.ct, r2sum, A1, A2, A3);
            else
                ni_visit_functions<NT, true>(tab, p.ntsf, pr.ct, r2sum, [&](int pos, double val, double dval) {
                    const double cc = cw[pos];
                    A3 = fma(cc, val, A3);
                    A2 = fma(cc * tab.sorted[4 * pos], val, A2);
                    A1 = fma(cc, dval, A1);
                });
            ni_forget_lds();
            A1 *= pr.tfc * (1.0 / ANNP_CFLENGTH);
            A2 *= pr.tfc;
            const double rx = p.compat ? pr.rkm : pr.rgm;       // ni:737-738 vs lal_annp.cu:409-414
            const double fcj = pr.fcj, fck = pr.fck, dfcj = L.dfc[sa], dfck = L.dfc[sb];
            const double irj = pr.ij, irk = pr.ik;
            const double t3j_a = fck * dfcj * pr.fcjk, t3_g = fck * fcj * pr.dfcjk;
            const double t3k_a = fcj * dfck * pr.fcjk;
            double fj[3], fk[3];
#pragma unroll
            for (int d = 0; d < 3; d++) {
                const double ej = pr.xj[d] * irj, ek = pr.xk[d] * irk, gg = (pr.xk[d] - pr.xj[d]) * pr.ig;
                const double dctj = (-ek + pr.ct * ej) * irj;     // ni:674
                const double dctk = (-ej + pr.ct * ek) * irk;
                const double t2j = 2.0 * (rx * gg - pr.rjm * ej), t2k = -2.0 * (pr.rkm * ek + rx * gg);
                const double t3j = t3_g * gg - t3j_a * ej, t3k = -(t3k_a * ek + t3_g * gg);
                fj[d] = A1 * dctj - A2 * t2j + A3 * t3j;
                fk[d] = A1 * dctk - A2 * t2k + A3 * t3k;
            }
            atomicAdd(&L.a0[sa], fj[0]); atomicAdd(&L.a1[sa], fj[1]); atomicAdd(&L.a2[sa], fj[2]);
            atomicAdd(&L.a0[sb], fk[0]); atomicAdd(&L.a1[sb], fk[1]); atomicAdd(&L.a2[sb], fk[2]);
        }
    }
    wave_lds_sync();
    double fi0 = 0.0, fi1 = 0.0, fi2 = 0.0;
    // one neighbour's total (the radial part was there before the pair loop's sums), handed to the table and to the centre
    for (int a = l; a < nmax; a += NI_GL) {
        if (a < nl) {
            const int s = sbase + a;
            const double g0 = L.a0[s], g1 = L.a1[s], g2 = L.a2[s];
            ni_table_add(L, p.f, L.sl[s], L.j[s], -g0 * ANNP_CFFORCE, -g1 * ANNP_CFFORCE, -g2 * ANNP_CFFORCE);       // ni:186-189
            fi0 += g0; fi1 += g1; fi2 += g2;
        }
    }
    // group sums (a group is a DPP row: four row shifts leave its sum in its last lane) -> the centre atom
    fi0 = row16_sum_to_last(fi0); fi1 = row16_sum_to_last(fi1); fi2 = row16_sum_to_last(fi2);
    const int i = L.ci[g];
    if (l == NI_GL - 1 && i >= 0) ni_table_add(L, p.f, L.cs[g], i, fi0 * ANNP_CFFORCE, fi1 * ANNP_CFFORCE, fi2 * ANNP_CFFORCE);
    if (VIRIAL) {       // a sweep of its own over the records (with the forces' it asked for more registers than three waves per SIMD leave)
        double v0 = 0.0, v1 = 0.0, v2 = 0.0, v3 = 0.0, v4 = 0.0, v5 = 0.0;
        ni_forget_lds();
        for (int a = l; a < nmax; a += NI_GL) {
            if (a < nl) {       // the reference tallies the un-converted force (ni:190-198)
                const int s = sbase + a;
                const double g0 = L.a0[s], g1 = L.a1[s], g2 = L.a2[s];
                const double d0 = L.dx[s], d1 = L.dy[s], d2 = L.dz[s];
                const double w0 = d0 * g0, w1 = d1 * g1, w2 = d2 * g2, w3 = d0 * g1, w4 = d0 * g2, w5 = d1 * g2;
                v0 += w0; v1 += w1; v2 += w2; v3 += w3; v4 += w4; v5 += w5;
                if (p.vatom) {
                    double *vj = p.vatom + 6 * (size_t)L.j[s];
                    atomicAdd(vj + 0, 0.5 * w0); atomicAdd(vj + 1, 0.5 * w1); atomicAdd(vj + 2, 0.5 * w2);
                    atomicAdd(vj + 3, 0.5 * w3); atomicAdd(vj + 4, 0.5 * w4); atomicAdd(vj + 5, 0.5 * w5);
                }
            }
        }
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) {
            v0 += __shfl_xor(v0, off, 64); v1 += __shfl_xor(v1, off, 64); v2 += __shfl_xor(v2, off, 64);
            v3 += __shfl_xor(v3, off, 64); v4 += __shfl_xor(v4, off, 64); v5 += __shfl_xor(v5, off, 64);
        }
        if (l == 0 && i >= 0 && p.vatom) {
            double *vi = p.vatom + 6 * (size_t)i;
            atomicAdd(vi + 0, 0.5 * v0); atomicAdd(vi + 1, 0.5 * v1); atomicAdd(vi + 2, 0.5 * v2);
            atomicAdd(vi + 3, 0.5 * v3); atomicAdd(vi + 4, 0.5 * v4); atomicAdd(vi + 5, 0.5 * v5);
        }
        if (p.virial) {
#pragma unroll
            for (int off = 32; off >= 16; off >>= 1) {
                v0 += __shfl_xor(v0, off, 64); v1 += __shfl_xor(v1, off, 64); v2 += __shfl_xor(v2, off, 64);
                v3 += __shfl_xor(v3, off, 64); v4 += __shfl_xor(v4, off, 64); v5 += __shfl_xor(v5, off, 64);
            }
            if (lane == 0) {
                double *vr = virial_row(p.virial);
                atomicAdd(&vr[0], v0); atomicAdd(&vr[1], v1); atomicAdd(&vr[2], v2);
                atomicAdd(&vr[3], v3); atomicAdd(&vr[4], v4); atomicAdd(&vr[5], v5);
            }
        }
    }
    wave_lds_sync();            // the next group of the run reuses the records
    }
    // ---- the run's force table: one global atomic per distinct atom and component (three neighbouring lanes per atom) ----------
    wave_lds_sync();
    for (int k = lane0; k < 3 * NI_TSLOTS; k += 64) {
        const int sl = k / 3;
        const int j = L.tkey[sl];
        if (j >= 0) atomicAdd(&p.f[3 * (size_t)j + (k - 3 * sl)], L.tacc[k]);
    }
    // ---- 5. energy and the in-cutoff maximum: one atomic per wave each ---------------------------------------------------------
    if (q.eng) {
        const double e = (esum[0] + esum[1]) + (esum[2] + esum[3]);
        if (lane0 == 0 && e != 0.0) atomicAdd(q.eng, e);
    }
    if (lane0 == 0 && nmax_run > 0) atomicMax(q.nmax_word, nmax_run);
}

// ---- launches ----------------------------------------------------------------------------------------------------------------
template <bool VIR>
inline void ni_launch_fused_t(const NiFusedArgs &a, NiShape sh, hipStream_t s)
{
    const int per_block = ANNP_WAVES_PER_BLOCK * NI_GA * NI_RUN;
    const int blocks = (a.n.inum + per_block - 1) / per_block;
    if (ni_is_shipped_shape(a.n, sh)) {
        if (a.n.n_cap <= NI_CAP_FIXED) {        // the capacity compiled in, as in the force pass
            NiFusedArgs c = a;
            c.n.n_cap = NI_CAP_FIXED;
            hipLaunchKernelGGL((annp_ni_fused<NI_SHIPPED, VIR, false, NI_CAP_FIXED>), dim3(blocks), dim3(256), ni_fused_lds_block(NI_CAP_FIXED, false), s, c);
        } else hipLaunchKernelGGL((annp_ni_fused<NI_SHIPPED, VIR, false>), dim3(blocks), dim3(256), ni_fused_lds_block(a.n.n_cap, false), s, a);
    } else hipLaunchKernelGGL((annp_ni_fused<NI_GENERIC, VIR, false>), dim3(blocks), dim3(256), ni_fused_lds_block(a.n.n_cap, true), s, a);
}
inline void ni_launch_fused(const NiFusedArgs &a, NiShape sh, bool virial, hipStream_t s)
{
    if (virial) ni_launch_fused_t<true>(a, sh, s); else ni_launch_fused_t<false>(a, sh, s);
}
// the fix-up launch: a fixed small grid whose waves walk the queue (empty in the steady state: they leave at once)
inline void ni_launch_fused_fix(const NiFusedArgs &a, NiShape sh, bool virial, hipStream_t s)
{
    const bool shipped = ni_is_shipped_shape(a.n, sh);
    const size_t lds = ni_fused_lds_block(a.n.n_cap, !shipped);
    const int blocks = std::max(1, std::min(NI_FIX_BLOCKS, (a.n.ovf_cap + ANNP_WAVES_PER_BLOCK - 1) / ANNP_WAVES_PER_BLOCK));
    if (virial) {
        if (shipped) hipLaunchKernelGGL((annp_ni_fused<NI_SHIPPED, true, true>), dim3(blocks), dim3(256), lds, s, a);
        else hipLaunchKernelGGL((annp_ni_fused<NI_GENERIC, true, true>), dim3(blocks), dim3(256), lds, s, a);
    } else {
        if (shipped) hipLaunchKernelGGL((annp_ni_fused<NI_SHIPPED, false, true>), dim3(blocks), dim3(256), lds, s, a);
        else hipLaunchKernelGGL((annp_ni_fused<NI_GENERIC, false, true>), dim3(blocks), dim3(256), lds, s, a);
    }
}

// the kernels may ask for more than the default 64 KB of dynamic LDS
inline hipError_t ni_fused_set_lds_attributes()
{
    const int full = 160 * 1024;
    hipError_t e;
#define NI_ATTR(...) if ((e = hipFuncSetAttribute((const void *)__VA_ARGS__, hipFuncAttributeMaxDynamicSharedMemorySize, full)) != hipSuccess) return e
    NI_ATTR(annp_ni_fused<NI_SHIPPED, false, false, NI_CAP_FIXED>);
    NI_ATTR(annp_ni_fused<NI_SHIPPED, true, false, NI_CAP_FIXED>);
    NI_ATTR(annp_ni_fused<NI_SHIPPED, false, false>);
    NI_ATTR(annp_ni_fused<NI_SHIPPED, true, false>);
    NI_ATTR(annp_ni_fused<NI_GENERIC, false, false>);
    NI_ATTR(annp_ni_fused<NI_GENERIC, true, false>);
    NI_ATTR(annp_ni_fused<NI_SHIPPED, false, true>);
    NI_ATTR(annp_ni_fused<NI_SHIPPED, true, true>);
    NI_ATTR(annp_ni_fused<NI_GENERIC, false, true>);
    NI_ATTR(annp_ni_fused<NI_GENERIC, true, true>);
#undef NI_ATTR
    return hipSuccess;
}

}  // namespace annp
