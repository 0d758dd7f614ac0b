"""The LeastAllocated term of the score-table kernels by a saturating convert (round 14, simon_table.hip: la_term_sat_t): the select
`requested >= capacity ? 0 : (int)fma(-r, rc100, 100 + 2^-33)` is the unsigned conversion of the same fma where that conversion clamps negative
values, -inf and NaN to 0, as v_cvt_u32_f64 does.  A host program with its own main compares the two forms with std::fma -- rc100 as the
library forms it, RN(100 * RN(1 / cap)) -- under the address and undefined-behaviour sanitizers: the clamp is spelled out, no cast of a
negative or non-finite double is executed."""
import shutil
import subprocess
import textwrap

SRC = textwrap.dedent(r'''
    #include <cmath>
    #include <cstdint>
    #include <cstdio>
    #include <numeric>
    #include <vector>

    // v_cvt_u32_f64: truncation towards zero, negative values and NaN give 0, values beyond the range the largest unsigned
    static uint32_t cvt_u32_sat(double v) {
        if (!(v > 0.0)) return 0u;                       // negative, -0, -inf, NaN
        if (v >= 4294967296.0) return 0xFFFFFFFFu;
        return (uint32_t)v;
    }
    static const double C = 100.0 + 0x1.0p-33;
    static int by_select(double r, double cap, double rc100) { return r >= cap ? 0 : (int)std::fma(-r, rc100, C); }
    static int by_convert(double r, double rc100) { return (int)cvt_u32_sat(std::fma(-r, rc100, C)); }

    static long checked = 0;
    static int check(uint64_t cap, uint64_t r) {
        const double dc = (double)cap, rc100 = 100.0 * (1.0 / dc), dr = (double)r;
        ++checked;
        if (by_select(dr, dc, rc100) != by_convert(dr, rc100)) {
            std::printf("cap %llu r %llu: select %d convert %d\n", (unsigned long long)cap, (unsigned long long)r, by_select(dr, dc, rc100), by_convert(dr, rc100));
            return 1;
        }
        // below the capacity both are the exact floor(100 (cap - r) / cap)
        if (cap && r < cap && by_convert(dr, rc100) != (int)((cap - r) * 100 / cap)) { std::printf("cap %llu r %llu: not the floor\n", (unsigned long long)cap, (unsigned long long)r); return 1; }
        return 0;
    }

    int main() {
        const uint64_t LIM = 1ull << 31;
        std::vector<uint64_t> caps = {1, 2, 3, 7, 100, 101, 3989, 7993, 65537, 1000003, 16777213, 16777259, 1073741827ull, 2147483629ull, 2147483647ull, LIM};
        uint64_t x = 88172645463325252ull;
        for (int i = 0; i < 4000; ++i) {                 // pseudo-random capacities over every magnitude up to 2^31
            x ^= x << 13; x ^= x >> 7; x ^= x << 17;
            caps.push_back(1 + (x >> 11) % (LIM >> (i % 31)));
        }
        int bad = 0;
        for (uint64_t cap : caps) {
            std::vector<uint64_t> rs = {0, 1, cap / 2, cap - 1, cap, cap + 1, cap + 2, 2 * cap - 1, 2 * cap, 2 * cap + 1, 3 * cap + 7, 100 * cap, LIM - 1, LIM, 0xFFFFFFFFull};
            for (int i = 0; i < 64; ++i) {
                x ^= x << 13; x ^= x >> 7; x ^= x << 17;
                uint64_t r = (x >> 9) % (4 * cap + 5);   // from 0 to beyond r - cap > cap
                if (std::gcd(r, cap) != 1) r += 1;       // mostly coprime to the capacity: no exact quotients
                rs.push_back(r);
            }
            for (uint64_t q = 1; q < 100; ++q) { rs.push_back(cap * q / 100); rs.push_back(cap * q / 100 + 1); }   // around every integer step of the term
            for (uint64_t r : rs) bad += check(cap, r);
        }
        for (uint64_t r : {0ull, 1ull, 1000ull, (unsigned long long)LIM}) bad += check(0, r);   // cap = 0: rc100 = +inf, the fma -inf or NaN
        if (bad) return 1;
        std::printf("ok %ld\n", checked);
        return 0;
    }
''')


def test_saturating_convert_equals_the_select(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler (g++ or clang++) on the path"
    src = tmp_path / "la_term_sat.cpp"
    src.write_text(SRC)
    exe = tmp_path / "la_term_sat"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=undefined,address", "-fno-sanitize-recover=all", "-o", str(exe), str(src)])
    out = subprocess.check_output([str(exe)]).decode().split()
    assert out[0] == "ok" and int(out[1]) > 1_000_000
