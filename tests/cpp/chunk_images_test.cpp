// Drives aai::engine::chunk_images (csrc/aai_engine.hpp), the arithmetic behind the adjoint's scratch-and-chunk loop: how many images of a
// batch go through per round of launches.  Host code only, no device is touched.  Built with the host side under the address and
// undefined-behaviour sanitizers and run as a program of its own:
//   hipcc -std=c++17 -Xarch_host -fsanitize=address,undefined -I area_average_interpolation_amd/csrc tests/cpp/chunk_images_test.cpp -o chunk_images_test
// Every pinned value follows from the rule: min(batch, 65535 images that grid.z carries, 1 GiB of fp64 scratch / imageBytes), at least 1;
// imageBytes == 0 means that the launches take no scratch.
#include <climits>
#include <cstddef>
#include <cstdio>

#include "aai_engine.hpp"

using aai::engine::chunk_images;

static int bad = 0;
static void expect(int batch, size_t imageBytes, int want)
{
    const int got = chunk_images(batch, imageBytes);
    if (got != want) { std::printf("FAIL: chunk_images(%d, %zu) = %d, expected %d\n", batch, imageBytes, got, want); ++bad; }
}

int main()
{
    const size_t GiB = (size_t)1 << 30;
    // no scratch: grid.z alone
    expect(1, 0, 1);
    expect(65535, 0, 65535);
    expect(65536, 0, 65535);
    expect(65540, 0, 65535);
    expect(INT_MAX, 0, 65535);
    // an image beyond 1 GiB still goes through, alone
    expect(96, GiB + 1, 1);
    expect(1, GiB + 1, 1);
    expect(96, (size_t)-1, 1);
    expect(96, GiB, 1);
    // tiny images: grid.z cuts first (2^30 / 8 = 2^27 > 65535), or the batch
    expect(70000, 8, 65535);
    expect(65540, 12 * 10 * 8, 65535);
    expect(5, 8, 5);
    // the 1 GiB rule where it is smaller than both: 1000 x 1000 doubles -> 134 images, 433 x 433 x 3 doubles -> 238
    expect(96, (size_t)1000 * 1000 * 8, 96);
    expect(200, (size_t)1000 * 1000 * 8, (int)(GiB / ((size_t)1000 * 1000 * 8)));
    expect(200, (size_t)1000 * 1000 * 8, 134);
    expect(70000, (size_t)433 * 433 * 3 * 8, 238);
    expect(70000, GiB / 2, 2);
    expect(70000, GiB / 2 + 1, 1);
    expect(70000, GiB / 65535, 65535);          // 16384 bytes: 2^30 / 16384 = 65536 images, grid.z still cuts first
    expect(70000, GiB / 65535 + 1, 65532);      // 16385 bytes: 65532 images
    // every round takes at least one image; an empty batch runs no round at all (the loop's own bound)
    expect(0, 0, 1);
    expect(0, 8, 1);
    // a whole batch is covered by rounds of the chunk with no overflow of the image index
    for (int batch : {1, 65535, 65536, 131071, INT_MAX}) {
        const int chunk = chunk_images(batch, 0);
        long long done = 0, rounds = 0;
        for (long long b0 = 0; b0 < batch; b0 += chunk) { done += (batch - b0 < chunk ? batch - b0 : chunk); ++rounds; }
        if (done != batch || rounds != ((long long)batch + chunk - 1) / chunk) { std::printf("FAIL: rounds of batch %d\n", batch); ++bad; }
    }
    std::printf(bad ? "chunk_images: %d failed\n" : "chunk_images: all ok\n", bad);
    return bad ? 1 : 0;
}
