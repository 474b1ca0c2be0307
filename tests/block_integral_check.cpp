// Stand-alone check of the host side of option block_integral (kfsp_block_integral.h: block_integral_column, with
// kfsp_padm.cpp and nothing of the device).  Built by tests/test_block_integral_host.py under host-side ASan / UBSan.
// Reads cases from the file named on the command line -
//     mh rows ldh tau, then the ldh * mh doubles of H (column-major, hexadecimal floats)
// - and prints "g <rows values as hexadecimal floats>" per case, then "ok".
#include "kfsp_block_integral.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    std::FILE *f = std::fopen(argv[1], "r");
    if (!f) return 2;
    std::vector<double> work;
    int mh = 0, rows = 0, ldh = 0;
    double tau = 0.0;
    while (std::fscanf(f, "%d %d %d %la", &mh, &rows, &ldh, &tau) == 4) {
        if (mh < 1 || mh > 102 || rows < 1 || rows > mh || ldh < mh || ldh > 128) return 3;
        std::vector<double> H((size_t)ldh * mh);                  // exactly what the routine may read ...
        for (double &x : H)
            if (std::fscanf(f, "%la", &x) != 1) return 3;
        std::vector<double> g((size_t)rows);                      // ... and write: an overrun is the sanitizer's to find
        if (const int rc = kfsp::block_integral_column(6, mh, rows, tau, H.data(), ldh, g.data(), work)) {
            std::printf("rc %d\n", rc);
            return 1;
        }
        std::printf("g");
        for (double x : g) std::printf(" %a", x);
        std::printf("\n");
    }
    std::fclose(f);
    // refusals: nothing is read or written
    double one = 1.0;
    if (kfsp::block_integral_column(6, 0, 1, 1.0, &one, 1, &one, work) != -2) return 4;
    if (kfsp::block_integral_column(6, 2, 3, 1.0, &one, 2, &one, work) != -2) return 4;
    if (kfsp::block_integral_column(6, 2, 1, 1.0, &one, 1, &one, work) != -2) return 4;
    std::printf("ok\n");
    return 0;
}
