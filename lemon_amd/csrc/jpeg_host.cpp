// jpeg_host.cpp -- liblemon_jpeg_host.so: the JPEG host pass built with the host compiler alone (lemon_amd/build.py).  It links
// no HIP runtime, so a decode worker loads it with ctypes without touching torch or the GPU.  The PNG host entry points
// (png_abi.hpp: chunk parser, IDAT copy, the looped device schedule) live in the same library.
#include "jpeg_abi.hpp"
#include "png_abi.hpp"
