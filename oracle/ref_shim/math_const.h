// ref_shim: TEST INFRASTRUCTURE -- not LAMMPS, not the reference.  Written from the LAMMPS developer documentation
// (stable_2Aug2023) so that the reference CPU pair styles compile unmodified outside LAMMPS (oracle/Makefile, target ref).
// LAMMPS math_const.h: the constant the reference uses.
#ifndef LMP_REFSHIM_MATH_CONST_H
#define LMP_REFSHIM_MATH_CONST_H
namespace LAMMPS_NS {
namespace MathConst {
static constexpr double MY_PI = 3.14159265358979323846;
static constexpr double MY_2PI = 6.28318530717958647692;
static constexpr double MY_PI2 = 1.57079632679489661923;
}
}
#endif
