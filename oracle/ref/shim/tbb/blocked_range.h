// Stand-in for oneTBB's <tbb/blocked_range.h>: included, never used.
#pragma once
