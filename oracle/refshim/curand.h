/* refshim/curand.h -- the reference includes cuRAND's host header next to
 * the device one; everything it uses is in curand_kernel.h. */
#include "curand_kernel.h"
