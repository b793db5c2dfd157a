// The plain C++ half of csrc/erm_item_pass.hpp, driven by tests/test_item_pass_host.py (built with g++ -fsanitize=undefined -ftrapv):
//   item_pass_check chunk BYTES N CAP ...   one line per triple: item_pass_chunk(BYTES, N, CAP)
//   item_pass_check words                    per pass, four lines: the noun, the shard refusal, the engine's refusal of too few rows ("-": it has none) with the
//                                            fewest rows it needs, the farm chain's with the fewest rows it needs
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "erm_item_pass.hpp"

using namespace erm;

int main(int argc, char** argv)
{
    if (argc >= 2 && !strcmp(argv[1], "chunk")) {
        for (int a = 2; a + 2 < argc; a += 3) printf("%lld\n", (long long)item_pass_chunk(atoll(argv[a]), atoll(argv[a + 1]), atoll(argv[a + 2])));
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "words")) {
        for (int p = 0; p < N_ITEM_PASSES; ++p) {
            const ItemPassFacts& f = ITEM_PASSES[p];
            printf("%s\n%s\n", f.noun, item_pass_on_shard(p).c_str());
            printf("%d %s\n", f.engine_rows, f.engine_rows > 0 ? item_pass_needs_rows(p).c_str() : "-");
            printf("%d %s\n", f.farm_rows, item_pass_needs_rows(p).c_str());
        }
        return 0;
    }
    fprintf(stderr, "usage: item_pass_check chunk BYTES N CAP ... | words\n");
    return 2;
}
