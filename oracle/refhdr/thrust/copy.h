// TEST INFRASTRUCTURE: stands in for <thrust/copy.h>; see device_ptr.h.
#pragma once
#include "device_ptr.h"
