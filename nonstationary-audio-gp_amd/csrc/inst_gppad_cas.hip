// one group of kernel instantiations of libnagp.so: the GPPAD cascade objective (nagp_gppad.hpp, V = 1)
#include "nagp_gppad.hpp"
NAGP_LIST_GPPAD_CAS(template __global__)
