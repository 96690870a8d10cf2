// one group of kernel instantiations of libnagp.so: the joint draws of a full-covariance EP run (nagp_epsample.hpp)
#include "nagp_epsample.hpp"
NAGP_LIST_EPSAMPLE(template __global__)
