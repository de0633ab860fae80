// jpeg_host.cpp -- liblemon_jpeg_host.so: the JPEG host pass built with the host compiler alone (lemon_amd/build.py).  It links
// no HIP runtime, so a decode worker loads it with ctypes without touching torch or the GPU.
#include "jpeg_abi.hpp"
