// ref_shim: TEST INFRASTRUCTURE -- not LAMMPS, not the reference.  Written from the LAMMPS developer documentation
// (stable_2Aug2023) so that the reference CPU pair styles compile unmodified outside LAMMPS (oracle/Makefile, target ref).
// LAMMPS math_extra.h: dot3 and scale3, the two helpers the reference calls.
#ifndef LMP_REFSHIM_MATH_EXTRA_H
#define LMP_REFSHIM_MATH_EXTRA_H
namespace LAMMPS_NS {
namespace MathExtra {
inline double dot3(const double *v1, const double *v2) { return v1[0] * v2[0] + v1[1] * v2[1] + v1[2] * v2[2]; }
inline void scale3(double s, const double *v, double *ans) { ans[0] = s * v[0]; ans[1] = s * v[1]; ans[2] = s * v[2]; }
}
}
#endif
