// one group of kernel instantiations of libnagp.so: the filterbank spectrum-fit objective (nagp_pstft.hpp)
#include "nagp_pstft.hpp"
NAGP_LIST_PSTFT(template __global__)
