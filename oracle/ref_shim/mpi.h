// ref_shim: TEST INFRASTRUCTURE -- not LAMMPS, not the reference.  Written from the LAMMPS developer documentation
// (stable_2Aug2023) so that the reference CPU pair styles compile unmodified outside LAMMPS (oracle/Makefile, target ref).
// A serial stand-in for mpi.h: one rank, so a broadcast from rank 0 leaves the buffer as it is.
#ifndef LMP_REFSHIM_MPI_H
#define LMP_REFSHIM_MPI_H
typedef int MPI_Comm;
typedef int MPI_Datatype;
#define MPI_COMM_WORLD 0
#define MPI_INT 1
#define MPI_DOUBLE 2
#define MPI_CHAR 3
#define MPI_FLOAT 4
#define MPI_SUCCESS 0
inline int MPI_Bcast(void *, int, MPI_Datatype, int, MPI_Comm) { return MPI_SUCCESS; }
#endif
