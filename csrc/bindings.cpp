// PyTorch bindings for the distriflow_amd gfx950 kernels (module distriflow_amd._C): each
// csrc/bindings_*.cpp validates and launches one topic's kernels and registers them here.  (No torch
// header in this file: parsing them is most of a bindings translation unit's compile time.)
#include <pybind11/pybind11.h>

#include "native_runtime.h"

namespace dfa_py {
void bind_comm(pybind11::module_& m);    // bindings_fused.cpp: P2PComm, PSComm (bindings_comm.h)
void bind_layers(pybind11::module_& m);  // bindings_layers.cpp: single-kernel layers, BatchNorm, optimizers
void bind_fused(pybind11::module_& m);   // bindings_fused.cpp: conv+pool, dense heads, kcnn, lenet_train
}  // namespace dfa_py

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "distriflow_amd native kernels (gfx950 / MI355X) and runtime";
  dfa_py::bind_comm(m);  // first: lenet_train's signature names P2PComm / PSComm
  dfa_py::bind_layers(m);
  dfa_py::bind_fused(m);
  dfa::register_runtime(m);
}
