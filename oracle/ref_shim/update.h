// ref_shim: TEST INFRASTRUCTURE -- not LAMMPS, not the reference.  Written from the LAMMPS developer documentation
// (stable_2Aug2023) so that the reference CPU pair styles compile unmodified outside LAMMPS (oracle/Makefile, target ref).
// LAMMPS update.h: the reference includes it and uses nothing from it (NeighConst lives in neighbor.h of tests/lammps_mock).
#ifndef LMP_REFSHIM_UPDATE_H
#define LMP_REFSHIM_UPDATE_H
#endif
