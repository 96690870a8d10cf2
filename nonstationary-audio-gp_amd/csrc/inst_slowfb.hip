// one group of kernel instantiations of libnagp.so: the exact filterbank smoother with per-step noise (nagp_slowfb.hpp)
#include "nagp_slowfb.hpp"
NAGP_LIST_SLOWFB(template __global__)
