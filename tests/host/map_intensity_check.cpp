// Host check of sonar_slam_amd/csrc/sfe_map_intensity.h, the per-cell expression of the published intensity mosaic:
// writes sfe_map_intensity_value(I, cnt) for cnt = 0 .. max_cnt and, for each cnt, I = 0 .. 255 * max(cnt, 1), as int8 bytes
// in that order to the file named on the command line; tests/test_mapping_intensity_host.py holds them to numpy's
// np.int8(np.round(I / 255.0 * 100.0 / cnt)).
//   g++ -std=c++17 -O1 -Wall -Wextra -Werror tests/host/map_intensity_check.cpp -o map_intensity_check
//   (for whoever changes the header: add -fsanitize=address,undefined)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../sonar_slam_amd/csrc/sfe_map_intensity.h"

int main(int argc, char **argv)
{
    if (argc != 3) {
        fprintf(stderr, "usage: %s max_cnt out_file\n", argv[0]);
        return 2;
    }
    const int max_cnt = atoi(argv[1]);
    if (max_cnt < 1 || max_cnt > 65535)
        return 2;
    std::vector<int8_t> out;
    for (int cnt = 0; cnt <= max_cnt; ++cnt)
        for (uint32_t I = 0; I <= 255u * (uint32_t)(cnt ? cnt : 1); ++I)
            out.push_back(sfe_map_intensity_value(I, (uint16_t)cnt));
    // the ties that tell half-even from half-up
    if (sfe_map_intensity_value(51, 8) != 2 || sfe_map_intensity_value(255, 8) != 12 || sfe_map_intensity_value(153, 8) != 8 ||
        sfe_map_intensity_value(357, 8) != 18 || sfe_map_intensity_value(7, 0) != -1) {
        fprintf(stderr, "map_intensity_check: a tie is rounded wrongly\n");
        return 1;
    }
    FILE *f = fopen(argv[2], "wb");
    if (!f || fwrite(out.data(), 1, out.size(), f) != out.size() || fclose(f) != 0)
        return 1;
    printf("map_intensity_check: ok, %zu values\n", out.size());
    return 0;
}
