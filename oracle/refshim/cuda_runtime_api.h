/* refshim/cuda_runtime_api.h -- see cuda_runtime.h */
#include "cuda_runtime.h"
