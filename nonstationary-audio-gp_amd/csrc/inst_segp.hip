// one group of kernel instantiations of libnagp.so: the modulator prior fit objective (nagp_segp.hpp)
#include "nagp_segp.hpp"
NAGP_LIST_SEGP(template __global__)
