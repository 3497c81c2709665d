// TEST INFRASTRUCTURE: stands in for <thrust/device_new.h>; see device_ptr.h.
#pragma once
#include "device_ptr.h"
