// ref_driver: TEST INFRASTRUCTURE -- not LAMMPS, not the reference, not the product.
// Plays LAMMPS around ONE object of a reference CPU pair style so that its own double-precision arithmetic can be run
// outside LAMMPS and its outputs committed as data (tests/golden/make_ref_golden.py).  The reference's header is not
// named here: oracle/Makefile force-includes it (-include) and says which class it declares:
//   -DREF_CLASS=PairANNP     -DREF_KIND=0   annp-gpu-lammps/fe_v2 (and fe): Chebyshev descriptor
//   -DREF_CLASS=PairANNP     -DREF_KIND=1   annp-gpu-lammps/ni: Behler G2/G4
//   -DREF_CLASS=PairANNA_ADP -DREF_KIND=2   anna-gpu-lammps/bcc_fe
// The LAMMPS surface comes from oracle/ref_shim/ and tests/lammps_mock/.
//
//   ref_driver CASE OUT        (what the reference prints goes to stdout: the caller sends it to a log)
//
// CASE (little endian, no padding): char magic[8] = "ANNPREF1"; int32 len + potential path; int32 ntypes, then per type
// int32 len + element name; int32 nlocal, nall, newton_pair, eflag, vflag, ncalls; double x[nall][3]; int32 type[nall];
// int32 inum; int32 ilist[inum]; int32 numneigh[nall]; int64 first[nall]; int64 total; int32 neigh[total] -- the full
// list in CSR form, rows indexed by atom, entries may carry LAMMPS' special bits.
// OUT: records {int32 len + name; char 'd' | 'i'; int32 ndim; int64 shape[ndim]; data}:
//   parsed/...   what read_file left in params[0] (scalars, normalisation rows, symmetry-function coefficients, every
//                weight and bias block as allocated, per element), map[1..ntypes], cutmax
//   callN/...    after the N-th compute(): f [nall][3] (ghost rows included), eng_vdwl, eatom [nall], virial [6],
//                vatom [nall][6]; atom->f is cleared before each call, as LAMMPS' integrator does
//   final/...    the normalisation rows once more after the last call (ni: compute() changes sf_max in place)
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "atom.h"
#include "comm.h"
#include "error.h"
#include "force.h"
#include "memory.h"
#include "neigh_list.h"
#include "neighbor.h"
#include "pair.h"

using namespace LAMMPS_NS;

namespace {

struct Out {
  FILE *fh;
  void head(const std::string &name, char kind, std::initializer_list<int64_t> shape)
  {
    const int32_t n = (int32_t) name.size(), nd = (int32_t) shape.size();
    fwrite(&n, 4, 1, fh);
    fwrite(name.data(), 1, name.size(), fh);
    fwrite(&kind, 1, 1, fh);
    fwrite(&nd, 4, 1, fh);
    for (int64_t s : shape) fwrite(&s, 8, 1, fh);
  }
  void d(const std::string &name, const double *v, std::initializer_list<int64_t> shape)
  {
    head(name, 'd', shape);
    size_t n = 1;
    for (int64_t s : shape) n *= (size_t) s;
    if (n) fwrite(v, 8, n, fh);
  }
  void d1(const std::string &name, double v) { d(name, &v, {}); }
  void i(const std::string &name, const int *v, std::initializer_list<int64_t> shape)
  {
    head(name, 'i', shape);
    size_t n = 1;
    for (int64_t s : shape) n *= (size_t) s;
    if (n) fwrite(v, 4, n, fh);
  }
  void i1(const std::string &name, int v) { i(name, &v, {}); }
};

struct In {
  FILE *fh;
  template <typename T> T one()
  {
    T v;
    if (fread(&v, sizeof(T), 1, fh) != 1) fail();
    return v;
  }
  template <typename T> void many(T *v, size_t n)
  {
    if (n && fread(v, sizeof(T), n, fh) != n) fail();
  }
  std::string str()
  {
    const int32_t n = one<int32_t>();
    if (n < 0 || n > (1 << 16)) fail();
    std::string s((size_t) n, '\0');
    many(&s[0], (size_t) n);
    return s;
  }
  [[noreturn]] static void fail()
  {
    fprintf(stderr, "ref_driver: malformed case file\n");
    exit(3);
  }
};

// the pair style's protected state, reached the way a derived style would
class Probe : public REF_CLASS {
 public:
  explicit Probe(LAMMPS *lmp) : REF_CLASS(lmp) {}

  void dump_rows(Out &out, const std::string &p)
  {
    const auto &P = params[0];
#if REF_KIND == 0
    out.d(p + "norm0", P.sfnor_cov, {P.nsf});
    out.d(p + "norm1", P.sfnor_avg, {P.nsf});
#elif REF_KIND == 1
    out.d(p + "norm0", P.sf_min, {P.nsf});
    out.d(p + "norm1", P.sf_max, {P.nsf});
#else
    out.d(p + "gparams", P.gparams, {P.ngp});
#endif
  }

  void dump_params(Out &out, const std::string &p, int ntypes)
  {
    const auto &P = params[0];
    out.i1(p + "nelements", P.nelements);
    out.i1(p + "ntl", P.ntl);
    out.i1(p + "nhl", P.nhl);
    out.i1(p + "nnod", P.nnod);
    out.i1(p + "nsf", P.nsf);
    out.i1(p + "npsf", P.npsf);
    out.i1(p + "ntsf", P.ntsf);
    out.i1(p + "flagsym", P.flagsym);
    out.i(p + "flagact", P.flagact, {P.ntl - 1});
    out.d1(p + "cut", P.cut);
    out.d1(p + "cutmax", cutmax);
    out.i(p + "map", map + 1, {ntypes});      // types 1..ntypes (entry 0 of map[] is never written by the reference)
#if REF_KIND == 2
    out.i1(p + "nout", P.nout);
    out.i1(p + "ngp", P.ngp);
    out.d1(p + "e_base", P.e_base);
    out.d1(p + "e_scal", P.e_scal);
#else
    out.d1(p + "e_scale", P.e_scale);
    out.d1(p + "e_shift", P.e_shift);
    out.d1(p + "e_atom", P.e_atom);
#endif
    dump_rows(out, p);
#if REF_KIND == 1
    {
      std::vector<double> rad((size_t) P.npsf * 3), ang((size_t) P.ntsf * 4);
      for (int m = 0; m < P.npsf; m++)
        for (int c = 0; c < 3; c++) rad[(size_t) m * 3 + c] = P.sym_coerad[m][c];
      for (int m = 0; m < P.ntsf; m++)
        for (int c = 0; c < 4; c++) ang[(size_t) m * 4 + c] = P.sym_coeang[m][c];
      out.d(p + "sym_rad", rad.data(), {P.npsf, 3});
      out.d(p + "sym_ang", ang.data(), {P.ntsf, 4});
    }
#endif
    // every block as read_file allocated it: weights [ntl-1][nnod][nsf], biases [ntl-1][nnod], zero where nothing was read
    const int nl = P.ntl - 1;
    std::vector<double> W((size_t) P.nelements * nl * P.nnod * P.nsf), B((size_t) P.nelements * nl * P.nnod);
    std::vector<double> mass((size_t) P.nelements);
    std::vector<int> id((size_t) P.nelements);
    size_t w = 0, b = 0;
    for (int e = 0; e < P.nelements; e++) {
#if REF_KIND == 2
      double ***wa = P.all_anna[e].weight_all, ***ba = P.all_anna[e].bias_all;
#else
      double ***wa = P.all_annp[e].weight_all, ***ba = P.all_annp[e].bias_all;
#endif
      for (int l = 0; l < nl; l++) {
        for (int r = 0; r < P.nnod; r++)
          for (int c = 0; c < P.nsf; c++) W[w++] = wa[l][r][c];
        for (int c = 0; c < P.nnod; c++) B[b++] = ba[l][0][c];
      }
      mass[(size_t) e] = P.all_elem[e].mass;
      id[(size_t) e] = P.all_elem[e].id_elem;
      const std::string &name = P.all_elem[e].elements;
      std::vector<int> chars(name.begin(), name.end());
      out.i(p + "element" + std::to_string(e), chars.data(), {(int64_t) chars.size()});
    }
    out.d(p + "W", W.data(), {P.nelements, nl, P.nnod, P.nsf});
    out.d(p + "B", B.data(), {P.nelements, nl, P.nnod});
    out.d(p + "mass", mass.data(), {P.nelements});
    out.i(p + "id_elem", id.data(), {P.nelements});
  }
};

}    // namespace

int main(int argc, char **argv)
{
  if (argc != 3) {
    fprintf(stderr, "usage: %s CASE OUT\n", argv[0]);
    return 2;
  }
  In in{fopen(argv[1], "rb")};
  if (!in.fh) {
    perror(argv[1]);
    return 2;
  }
  char magic[8];
  in.many(magic, 8);
  if (std::string(magic, 8) != "ANNPREF1") In::fail();
  std::string potfile = in.str();
  const int ntypes = in.one<int32_t>();
  if (ntypes < 1 || ntypes > 64) In::fail();
  std::vector<std::string> names;
  for (int t = 0; t < ntypes; t++) names.push_back(in.str());
  const int nlocal = in.one<int32_t>(), nall = in.one<int32_t>(), newton_pair = in.one<int32_t>();
  const int eflag = in.one<int32_t>(), vflag = in.one<int32_t>(), ncalls = in.one<int32_t>();
  if (nlocal < 0 || nall < nlocal || ncalls < 0) In::fail();
  std::vector<double> x((size_t) nall * 3), f((size_t) nall * 3, 0.0);
  std::vector<int> type((size_t) nall);
  in.many(x.data(), x.size());
  in.many(type.data(), type.size());
  const int inum = in.one<int32_t>();
  if (inum < 0 || inum > nall) In::fail();
  std::vector<int> ilist((size_t) inum), numneigh((size_t) nall);
  std::vector<int64_t> first((size_t) nall);
  in.many(ilist.data(), ilist.size());
  in.many(numneigh.data(), numneigh.size());
  in.many(first.data(), first.size());
  const int64_t total = in.one<int64_t>();
  if (total < 0) In::fail();
  std::vector<int> neigh((size_t) total + 1);
  in.many(neigh.data(), (size_t) total);
  fclose(in.fh);
  for (int i = 0; i < nall; i++)
    if (numneigh[(size_t) i] < 0 || first[(size_t) i] < 0 || first[(size_t) i] + numneigh[(size_t) i] > total) In::fail();
  for (int64_t k = 0; k < total; k++)
    if ((neigh[(size_t) k] & NEIGHMASK) >= nall) In::fail();
  for (int i : ilist)
    if (i < 0 || i >= nall) In::fail();

  Memory memory;
  Error error;
  Atom atom;
  Neighbor neighbor;
  Comm comm;
  Force force;
  LAMMPS lmp;
  lmp.memory = &memory;
  lmp.error = &error;
  lmp.atom = &atom;
  lmp.neighbor = &neighbor;
  lmp.comm = &comm;
  lmp.force = &force;
  lmp.screen = stdout;
  force.newton = force.newton_pair = newton_pair;

  std::vector<double *> xrow((size_t) nall + 1), frow((size_t) nall + 1);
  for (int i = 0; i < nall; i++) {
    xrow[(size_t) i] = &x[(size_t) i * 3];
    frow[(size_t) i] = &f[(size_t) i * 3];
  }
  atom.ntypes = ntypes;
  atom.nlocal = nlocal;
  atom.nghost = nall - nlocal;
  atom.nmax = nall;
  atom.x = xrow.data();
  atom.f = frow.data();
  atom.type = type.data();

  std::vector<int *> firstneigh((size_t) nall + 1);
  for (int i = 0; i < nall; i++) firstneigh[(size_t) i] = neigh.data() + first[(size_t) i];
  NeighList list;
  list.inum = inum;
  list.ilist = ilist.data();
  list.numneigh = numneigh.data();
  list.firstneigh = firstneigh.data();

  Out out{fopen(argv[2], "wb")};
  if (!out.fh) {
    perror(argv[2]);
    return 2;
  }
  try {
    Probe *pair = new Probe(&lmp);        // never deleted: the reference's destructors free less than it allocates
    force.pair = pair;
    pair->settings(0, nullptr);
    std::vector<std::string> words = {"*", "*", potfile};
    words.insert(words.end(), names.begin(), names.end());
    std::vector<char *> arg;
    for (auto &w : words) arg.push_back(&w[0]);
    pair->coeff((int) arg.size(), arg.data());
    pair->dump_params(out, "parsed/", ntypes);
    pair->init();                          // init_style, then init_one for every type pair -> cutsq
    pair->list = &list;
    for (int c = 1; c <= ncalls; c++) {
      std::fill(f.begin(), f.end(), 0.0);
      pair->compute(eflag, vflag);
      fflush(stdout);
      const std::string p = "call" + std::to_string(c) + "/";
      out.d(p + "f", f.data(), {nall, 3});
      out.d1(p + "eng_vdwl", pair->eng_vdwl);
      if (pair->eflag_atom) out.d(p + "eatom", pair->eatom, {nall});
      out.d(p + "virial", pair->virial, {6});
      if (pair->vflag_atom) out.d(p + "vatom", nall ? pair->vatom[0] : nullptr, {nall, 6});
    }
    pair->dump_rows(out, "final/");
  } catch (const std::exception &e) {
    fflush(stdout);
    fprintf(stderr, "ref_driver: %s\n", e.what());
    fclose(out.fh);
    return 4;
  }
  fclose(out.fh);
  return 0;
}
