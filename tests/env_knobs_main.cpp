// Stand-alone host program for tests/test_env_knobs_host.py: the switch readers of csrc/common.hpp on every kind of value.
#include <stdio.h>

#include "../openseg3d_amd/csrc/common.hpp"

static int failures = 0;

#define EXPECT(expr, want)                                                           \
    do {                                                                             \
        const int got_ = (int)(expr);                                                \
        if (got_ != (want)) {                                                        \
            printf("%s:%d: %s = %d, expected %d\n", __FILE__, __LINE__, #expr, got_, (int)(want)); \
            ++failures;                                                              \
        }                                                                            \
    } while (0)

static void put(const char* value) {
    if (value)
        setenv("SEG3D_TEST_KNOB", value, 1);
    else
        unsetenv("SEG3D_TEST_KNOB");
}

int main() {
    const char* k = "SEG3D_TEST_KNOB";
    put(nullptr);  // unset: the default, whatever the range
    EXPECT(env_set(k), 0);
    EXPECT(env_int(k, 7), 7);
    EXPECT(env_int_in(k, 1, 64, 0), 0);
    EXPECT(env_int_in(k, 64, 4096, 512), 512);
    put("");  // set and empty reads as 0
    EXPECT(env_set(k), 1);
    EXPECT(env_int(k, 7), 0);
    EXPECT(env_int_in(k, 1, 64, 5), 5);
    EXPECT(env_int_in(k, 0, 64, 5), 0);
    put("abc");  // no leading number reads as 0
    EXPECT(env_set(k), 1);
    EXPECT(env_int(k, 7), 0);
    EXPECT(env_int_in(k, 64, 2147483647, 3072), 3072);
    put("0");
    EXPECT(env_set(k), 1);  // "set at all"
    EXPECT(env_int(k, 1), 0);
    put("12x");  // atoi: the leading number
    EXPECT(env_int(k, 7), 12);
    put("-3");
    EXPECT(env_int(k, 7), -3);
    EXPECT(env_int_in(k, 1, 64, 1), 1);  // below the range
    put("63");
    EXPECT(env_int_in(k, 64, 2147483647, 3072), 3072);
    put("1");
    EXPECT(env_int_in(k, 1, 64, 0), 1);  // the range's ends belong to it
    put("64");
    EXPECT(env_int_in(k, 1, 64, 0), 64);
    EXPECT(env_int_in(k, 64, 4096, 512), 64);
    put("65");
    EXPECT(env_int_in(k, 1, 64, 0), 0);  // above the range
    put("100000");
    EXPECT(env_int_in(k, 64, 2147483647, 3072), 100000);
    EXPECT(env_int_in(k, 64, 4096, 512), 512);
    if (!failures) printf("ok\n");
    return failures ? 1 : 0;
}
