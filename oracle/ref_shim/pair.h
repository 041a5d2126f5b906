// ref_shim: TEST INFRASTRUCTURE -- not LAMMPS, not the reference.  Written from the LAMMPS developer documentation
// (stable_2Aug2023) so that the reference CPU pair styles compile unmodified outside LAMMPS (oracle/Makefile, target ref).
// LAMMPS pair.h for the reference pair styles: every member tests/lammps_mock/pair.h declares (same names and
// semantics, so tests/lammps_mock/mock_lammps.cpp implements them for this class as well) plus what only the reference
// touches: map, nparams, comm_forward, ev_tally_xyz.  This header shadows the mock's pair.h on the include path of the
// reference binaries only; the adaptor's mock build never sees it.
#ifndef LMP_PAIR_H
#define LMP_PAIR_H
#include <cstring>
#include <string>

#include "mpi.h"
#include "pointers.h"
namespace LAMMPS_NS {
class NeighList;
class Pair : protected Pointers {
 public:
  double eng_vdwl = 0.0, eng_coul = 0.0;
  double virial[6] = {0, 0, 0, 0, 0, 0};
  double *eatom = nullptr, **vatom = nullptr;
  double cutforce = 0.0;
  double **cutsq = nullptr;
  int **setflag = nullptr;
  int restartinfo = 1, one_coeff = 0, manybody_flag = 0, no_virial_fdotr = 0;
  int allocated = 0, copymode = 0;
  int comm_forward = 0, comm_reverse = 0;
  NeighList *list = nullptr;
  int evflag = 0, eflag_either = 0, eflag_global = 0, eflag_atom = 0, vflag_either = 0, vflag_global = 0, vflag_atom = 0, vflag_fdotr = 0;
  int maxeatom = 0, maxvatom = 0;

  explicit Pair(LAMMPS *lmp) : Pointers(lmp) {}
  ~Pair() override;
  virtual void compute(int, int) = 0;
  virtual void settings(int, char **) = 0;
  virtual void coeff(int, char **) = 0;
  virtual void init_style();
  virtual double init_one(int, int) { return 0.0; }
  virtual double memory_usage();
  void init();
  void ev_init(int eflag, int vflag, int alloc = 1) { if (eflag || vflag) ev_setup(eflag, vflag, alloc); else ev_unset(); }
  void ev_setup(int, int, int alloc = 1);
  void ev_unset();
  void virial_fdotr_compute();
  // tally of one pair term (i, j) with force (fx, fy, fz) on i and separation del = x_i - x_j: ref_shim.cpp
  void ev_tally_xyz(int i, int j, int nlocal, int newton_pair, double evdwl, double ecoul, double fx, double fy, double fz,
                    double delx, double dely, double delz);

 protected:
  int nparams = 0, maxparam = 0;    // manybody styles: number of parameter sets
  int *map = nullptr;               // LAMMPS type -> element of the potential file, -1 = not mapped
};
enum { ENERGY_NONE = 0x00, ENERGY_GLOBAL = 0x01, ENERGY_ATOM = 0x02 };
enum { VIRIAL_NONE = 0x00, VIRIAL_PAIR = 0x01, VIRIAL_FDOTR = 0x02, VIRIAL_ATOM = 0x04, VIRIAL_CENTROID = 0x08 };
}
#endif
