/* host/query_ops.h on edge lines, as a stand-alone program (tests/test_clause_native.py builds it
 * with AddressSanitizer and UndefinedBehaviorSanitizer).  Every output buffer is allocated at
 * exactly the size the header promises to need, so a byte too many is a heap overflow. */
#include <stdio.h>

#include "query_ops.h"

static int failures;

#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

/* one line through qops_split_line, the three texts compared with what is expected */
static void line_case(const char* line, size_t len, int ops, int all, const char* must, size_t nm, const char* should,
                      size_t ns, const char* not_, size_t nx) {
    uint8_t* in = (uint8_t*)malloc(len ? len : 1);
    uint8_t* out[3];
    size_t n[3];
    for (int c = 0; c < 3; ++c) out[c] = (uint8_t*)malloc(len ? len : 1);
    if (len) memcpy(in, line, len);
    qops_split_line(in, len, ops, all, out, n);
    const char* want[3] = {must, should, not_};
    const size_t wn[3] = {nm, ns, nx};
    for (int c = 0; c < 3; ++c) {
        if (n[c] != wn[c] || (wn[c] && memcmp(out[c], want[c], wn[c]) != 0)) {
            printf("FAILED line \"%.*s\" (ops %d, all %d): text %d has %zu bytes, expected %zu\n", (int)(len < 40 ? len : 40), line,
                   ops, all, c, n[c], wn[c]);
            ++failures;
        }
        free(out[c]);
    }
    free(in);
}

#define L(s) s, sizeof(s) - 1

int main(void) {
    /* the operators themselves */
    line_case(L("+a b -c"), 1, 0, L("a"), L("b"), L("c"));
    line_case(L("+"), 1, 0, L(""), L("+"), L(""));                    /* a lone operator is a should token */
    line_case(L("-"), 1, 0, L(""), L("-"), L(""));
    line_case(L(" + \t-\n"), 1, 0, L(""), L("+ -"), L(""));
    line_case(L("++x"), 1, 0, L("+x"), L(""), L(""));                 /* only the first byte is an operator */
    line_case(L("-+x"), 1, 0, L(""), L(""), L("+x"));
    line_case(L("+-x --y"), 1, 0, L("-x"), L(""), L("-y"));
    line_case(L("a+b a-b"), 1, 0, L(""), L("a+b a-b"), L(""));        /* not at the token's start */
    line_case(L(""), 1, 0, L(""), L(""), L(""));                      /* an empty line */
    line_case(L(" \t\r\n\v\f"), 1, 0, L(""), L(""), L(""));
    line_case(L("+a +b"), 1, 0, L("a b"), L(""), L(""));              /* joined by one blank, in order */
    line_case(L("x\t\t+a  y\n-b +c z"), 1, 0, L("a c"), L("x y z"), L("b"));
    /* a NUL inside a token stays where it is */
    line_case(L("+a\0b c\0 -\0d"), 1, 0, L("a\0b"), L("c\0"), L("\0d"));
    line_case(L("+\0"), 1, 0, L("\0"), L(""), L(""));                 /* two bytes: an operator and a NUL */
    /* --query-all: every token without an operator is a must; without --query-ops none has one */
    line_case(L("a +b -c -"), 1, 1, L("a b -"), L(""), L("c"));
    line_case(L("a +b -c"), 0, 1, L("a +b -c"), L(""), L(""));
    line_case(L("a +b -c"), 0, 0, L(""), L("a +b -c"), L(""));        /* --min-match alone */
    /* a 70 KB token, with and without an operator, and no final newline */
    {
        const size_t n = 70u * 1024u;
        char* big = (char*)malloc(n + 3);
        memset(big, 'q', n + 3);
        big[0] = '+';
        line_case(big, n, 1, 0, big + 1, n - 1, L(""), L(""));
        big[0] = '-';
        line_case(big, n, 1, 0, L(""), L(""), big + 1, n - 1);
        big[0] = 'q';
        line_case(big, n, 1, 0, L(""), big, n, L(""));
        free(big);
    }
    /* a batch: line starts as the CLI cuts them (the newline stays in its line), the last line
     * without its newline, an empty line in the middle */
    {
        const char text[] = "+a b\n\n-c +d\0e f\n+";
        const uint64_t nb = sizeof(text) - 1;
        uint8_t* bytes = (uint8_t*)malloc(nb);
        memcpy(bytes, text, nb);
        const uint64_t off[5] = {0, 5, 6, 16, 17};
        uint8_t* tb[3];
        uint64_t tn[3], *to[3];
        CHECK(off[4] == nb);
        CHECK(qops_split_batch(bytes, off, 4, 1, 0, tb, tn, to) == 0);
        CHECK(tn[0] == 4 && memcmp(tb[0], "ad\0e", 4) == 0);
        CHECK(to[0][0] == 0 && to[0][1] == 1 && to[0][2] == 1 && to[0][3] == 4 && to[0][4] == 4);
        CHECK(tn[1] == 3 && memcmp(tb[1], "bf+", 3) == 0);
        CHECK(to[1][0] == 0 && to[1][1] == 1 && to[1][2] == 1 && to[1][3] == 2 && to[1][4] == 3);
        CHECK(tn[2] == 1 && tb[2][0] == 'c');
        CHECK(to[2][0] == 0 && to[2][2] == 0 && to[2][3] == 1 && to[2][4] == 1);
        for (int c = 0; c < 3; ++c) { free(tb[c]); free(to[c]); }
        /* no query at all */
        const uint64_t off0[1] = {0};
        CHECK(qops_split_batch(bytes, off0, 0, 1, 0, tb, tn, to) == 0);
        for (int c = 0; c < 3; ++c) {
            CHECK(tb[c] && to[c] && tn[c] == 0 && to[c][0] == 0);
            free(tb[c]);
            free(to[c]);
        }
        free(bytes);
    }
    if (failures) return 1;
    printf("ok\n");
    return 0;
}
