// one group of kernel instantiations of libnagp.so: the joint draws of the stationary filterbank (nagp_fbsample.hpp)
#include "nagp_fbsample.hpp"
NAGP_LIST_FBSAMPLE(template __global__)
