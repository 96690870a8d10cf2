// one group of kernel instantiations of libnagp.so: the fixed-point NMF (nagp_nmf.hpp)
#include "nagp_nmf.hpp"
NAGP_LIST_NMF(template __global__)
