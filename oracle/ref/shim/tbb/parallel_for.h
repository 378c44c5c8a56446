// Stand-in for oneTBB's <tbb/parallel_for.h>: the index form parallel_for(first, last, f), run serially.
#pragma once
#include "blocked_range.h"

namespace tbb {

template <typename Index, typename Function>
inline void parallel_for(Index first, Index last, const Function& f)
{
    for (Index i = first; i < last; ++i) f(i);
}

} // namespace tbb
