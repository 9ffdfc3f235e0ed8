// quartet_math.hpp -- the two figures every layer of the host shares and that need no device: C(x,4) and the QP-IC of three sums.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

namespace qsh {

inline uint64_t c4(uint64_t x) { return x < 4 ? 0 : x * (x - 1) * (x - 2) * (x - 3) / 24; }   // C(x,4)

// QuartetScoreComputer.hpp:135-159 with the host libm
inline double raw_log_score(size_t q1, size_t q2, size_t q3) {
    if (q1 == 0 && q2 == 0 && q3 == 0) return 0;
    size_t sum = q1 + q2 + q3;
    double p1 = (double)q1 / sum, p2 = (double)q2 / sum, p3 = (double)q3 / sum;
    double qic = 1;
    if (p1 != 0) qic += p1 * std::log(p1) / std::log(3);
    if (p2 != 0) qic += p2 * std::log(p2) / std::log(3);
    if (p3 != 0) qic += p3 * std::log(p3) / std::log(3);
    return (q1 < q2 || q1 < q3) ? qic * -1 : qic;
}

} // namespace qsh
