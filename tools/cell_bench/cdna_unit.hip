// k_cdna for tools/cell_bench/kernel_bench.hip, in a translation unit of its own: ccsx_cdna.hip and ccsx_cell.hip name the helpers of their unnamed namespaces alike
#include "../../ccs_amd/csrc/ccsx_cdna.hip"
