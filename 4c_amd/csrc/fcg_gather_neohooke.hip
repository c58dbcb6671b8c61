// fcg_gather_neohooke.hip -- the ElastHyper/CoupNeoHooke instantiations of the node-row gather
// (fcg_gather.hip) in a translation unit of their own, so that they can be compiled without the
// machine loop-invariant code motion (see launch_gather_h8_neohooke in fcg_gather.hip and the
// 4c_amd/Makefile rule).
#define FCG_GATHER_NEOHOOKE_TU
#include "fcg_gather.hip"
