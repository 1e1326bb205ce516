// Stand-alone host check of linear-programming_amd/csrc/xwide.h (tests/test_exact_wide_host.py compiles it
// with the host compiler and -fsanitize=address,undefined and runs it as a program).  One request per input
// line, one answer per output line; wide values are hexadecimal two's complement, 64 digits for 256 bits and
// 128 for 512, 64-bit values decimal:
//   mul A B     -> "ovf" | "ok P"     the product in 256 bits (xw_mul_ovf)
//   full A B    -> P                  the 512-bit product (xw_mul)
//   div A d     -> Q R                A / d and A % d as C has them, d > 0 (xw_divmod_small)
//   lcm d1 ..   -> "ovf" | "ok L"     the LCM of the chain, from 1 (xw_lcm_small)
//   sym A       -> 0 | 1              A is inside the symmetric range (what x_fits asks at 256 bits)
//   fit W       -> "no" | "ok A"      the 512-bit W as a 256-bit value inside the symmetric range (xw_fit)
//   cmp A B     -> lt eq              A < B and A == B, signed
#include "../linear-programming_amd/csrc/xwide.h"

#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

using namespace mi355x;

template <int N> static XWide<N> parse(const std::string &s)
{
    XWide<N> r;
    for (int i = 0; i < N; ++i) r.l[i] = std::stoull(s.substr(s.size() - 16 * (i + 1), 16), nullptr, 16);
    return r;
}
template <int N> static std::string show(const XWide<N> &x)
{
    std::string s;
    char buf[17];
    for (int i = N - 1; i >= 0; --i) {
        snprintf(buf, sizeof buf, "%016llx", (unsigned long long)x.l[i]);
        s += buf;
    }
    return s;
}

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string op, a, b;
        in >> op;
        if (op == "mul") {
            in >> a >> b;
            XWide<4> r;
            if (xw_mul_ovf(parse<4>(a), parse<4>(b), &r)) std::cout << "ok " << show(r) << "\n";
            else std::cout << "ovf\n";
        } else if (op == "full") {
            in >> a >> b;
            std::cout << show(xw_mul(parse<4>(a), parse<4>(b))) << "\n";
        } else if (op == "div") {
            long long d;
            in >> a >> d;
            int64_t rem = 0;
            const XWide<4> q = xw_divmod_small(parse<4>(a), (int64_t)d, &rem);
            std::cout << show(q) << " " << (long long)rem << "\n";
        } else if (op == "lcm") {
            XWide<4> l = 1;
            bool ok = true;
            long long d;
            while (ok && in >> d) ok = xw_lcm_small(l, (int64_t)d, &l);
            if (ok) std::cout << "ok " << show(l) << "\n";
            else std::cout << "ovf\n";
        } else if (op == "sym") {
            in >> a;
            std::cout << (xw_is_min(parse<4>(a)) ? 0 : 1) << "\n";
        } else if (op == "fit") {
            in >> a;
            XWide<4> r;
            if (xw_fit<4>(parse<8>(a), &r)) std::cout << "ok " << show(r) << "\n";
            else std::cout << "no\n";
        } else if (op == "cmp") {
            in >> a >> b;
            std::cout << (parse<4>(a) < parse<4>(b) ? 1 : 0) << " " << (parse<4>(a) == parse<4>(b) ? 1 : 0) << "\n";
        } else {
            std::cout << "?\n";
        }
    }
    return 0;
}
