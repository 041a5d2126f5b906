// ref_shim: TEST INFRASTRUCTURE -- not LAMMPS, not the reference.  Written from the LAMMPS developer documentation
// (stable_2Aug2023) so that the reference CPU pair styles compile unmodified outside LAMMPS (oracle/Makefile, target ref).
// LAMMPS math_special.h: the reference opens the namespace and calls nothing from it.
#ifndef LMP_REFSHIM_MATH_SPECIAL_H
#define LMP_REFSHIM_MATH_SPECIAL_H
namespace LAMMPS_NS {
namespace MathSpecial {
inline double square(double x) { return x * x; }
}
}
#endif
