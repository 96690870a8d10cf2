// one group of kernel instantiations of libnagp.so: the objective of the conjugate-gradient NMF with temporal priors (nagp_nmf_temp.hpp)
#include "nagp_nmf_temp.hpp"
NAGP_LIST_NMFT(template __global__)
