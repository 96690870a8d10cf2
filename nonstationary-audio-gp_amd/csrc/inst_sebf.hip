// one group of kernel instantiations of libnagp.so: the squared-exponential basis-function convolution and its reductions (nagp_sebf.hpp)
#include "nagp_sebf.hpp"
NAGP_LIST_SEBF(template __global__)
