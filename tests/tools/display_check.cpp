// display_check — the curves of loupiote_amd/csrc/display_math.h (SPEC §30) on the CPU, for tests/test_display.py.
// stdin: one case per line, "op gain_bits r_bits g_bits b_bits" (the operator, then the bit patterns of the gain and of one pixel's mean, in hex);
// stdout: per case the bit patterns of the three values the transform hands to the sRGB encoding.  A line "bin y_bits" prints the meter's bin of a
// luminance, or -1 where the pixel is skipped.  Built by g++ with -ffp-contract=off: the header is plain C++.
#include <cstdio>
#include <cstring>

#include "display_math.h"

using namespace lptd;

static float from_bits(unsigned u) { float f; memcpy(&f, &u, sizeof f); return f; }

int main() {
    char line[256];
    while (fgets(line, sizeof line, stdin)) {
        unsigned op, g, r, gg, b;
        if (sscanf(line, "bin %x", &r) == 1) {
            uint32_t bin = 0;
            printf("%d\n", meter_bin(from_bits(r), bin) ? (int)bin : -1);
            continue;
        }
        if (sscanf(line, "%u %x %x %x %x", &op, &g, &r, &gg, &b) != 5 || op >= kDisplayOps) { fprintf(stderr, "display_check: bad line: %s", line); return 2; }
        rgb3 m;
        m.r = from_bits(r); m.g = from_bits(gg); m.b = from_bits(b);
        const float gain = from_bits(g);
        const rgb3 o = op == kDisplayClamp ? display_transform<kDisplayClamp>(m, gain) : op == kDisplayPbrNeutral ? display_transform<kDisplayPbrNeutral>(m, gain) : display_transform<kDisplayAces>(m, gain);
        printf("%08x %08x %08x\n", disp_bits(o.r), disp_bits(o.g), disp_bits(o.b));
    }
    return 0;
}
