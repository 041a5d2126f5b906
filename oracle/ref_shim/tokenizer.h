// ref_shim: TEST INFRASTRUCTURE -- not LAMMPS, not the reference.  Written from the LAMMPS developer documentation
// (stable_2Aug2023) so that the reference CPU pair styles compile unmodified outside LAMMPS (oracle/Makefile, target ref).
// LAMMPS tokenizer.h: the exception type the reference's read_file catches (nothing in it throws one).
#ifndef LMP_REFSHIM_TOKENIZER_H
#define LMP_REFSHIM_TOKENIZER_H
#include <exception>
#include <string>
namespace LAMMPS_NS {
class TokenizerException : public std::exception {
  std::string message;
 public:
  explicit TokenizerException(const std::string &msg) : message(msg) {}
  const char *what() const noexcept override { return message.c_str(); }
};
}
#endif
