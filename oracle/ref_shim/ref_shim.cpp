// ref_shim: TEST INFRASTRUCTURE -- not LAMMPS, not the reference.  Written from the LAMMPS developer documentation
// (stable_2Aug2023) so that the reference CPU pair styles compile unmodified outside LAMMPS (oracle/Makefile, target ref).
// Pair::ev_tally_xyz as the developer documentation describes it: the energy of a pair term goes to the global
// accumulators (whole with newton_pair on, otherwise one half per owned atom of the pair) and in halves to eatom[i] and
// eatom[j]; the virial term v = del (x) f likewise to virial[6] and in halves to vatom[i], vatom[j].  A per-atom share is
// tallied when newton_pair is on or the atom is owned (index < nlocal).
#include "pair.h"

using namespace LAMMPS_NS;

void Pair::ev_tally_xyz(int i, int j, int nlocal, int newton_pair, double evdwl, double ecoul, double fx, double fy, double fz,
                        double delx, double dely, double delz)
{
  const bool own_i = newton_pair || i < nlocal, own_j = newton_pair || j < nlocal;
  if (eflag_either) {
    if (eflag_global) {
      if (newton_pair) {
        eng_vdwl += evdwl;
        eng_coul += ecoul;
      } else {
        if (i < nlocal) { eng_vdwl += 0.5 * evdwl; eng_coul += 0.5 * ecoul; }
        if (j < nlocal) { eng_vdwl += 0.5 * evdwl; eng_coul += 0.5 * ecoul; }
      }
    }
    if (eflag_atom) {
      const double half = 0.5 * (evdwl + ecoul);
      if (own_i) eatom[i] += half;
      if (own_j) eatom[j] += half;
    }
  }
  if (vflag_either) {
    const double v[6] = {delx * fx, dely * fy, delz * fz, delx * fy, delx * fz, dely * fz};
    if (vflag_global) {
      if (newton_pair) {
        for (int k = 0; k < 6; k++) virial[k] += v[k];
      } else {
        if (i < nlocal) for (int k = 0; k < 6; k++) virial[k] += 0.5 * v[k];
        if (j < nlocal) for (int k = 0; k < 6; k++) virial[k] += 0.5 * v[k];
      }
    }
    if (vflag_atom) {
      if (own_i) for (int k = 0; k < 6; k++) vatom[i][k] += 0.5 * v[k];
      if (own_j) for (int k = 0; k < 6; k++) vatom[j][k] += 0.5 * v[k];
    }
  }
}
