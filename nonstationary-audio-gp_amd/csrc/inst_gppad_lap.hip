// one group of kernel instantiations of libnagp.so: the Laplace step of GPPAD (nagp_gppad_lap.hpp)
#include "nagp_gppad_lap.hpp"
NAGP_LIST_GPPAD_LAP(template __global__)
