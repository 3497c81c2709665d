// TEST INFRASTRUCTURE: stands in for <thrust/swap.h>; see device_ptr.h.
#pragma once
#include "device_ptr.h"
