// one group of kernel instantiations of libnagp.so: the GPPAD envelope objective (nagp_gppad.hpp)
#include "nagp_gppad.hpp"
NAGP_LIST_GPPAD(template __global__)
