// tile_lds (amof_amd/csrc/rdf_select.h) for tests/test_tile_lds_cpu.py: one line "nbins queue defer" per request on
// stdin, one line "unplanned planned" on stdout.
#include <stdio.h>

#include "../../amof_amd/csrc/rdf_select.h"

int main()
{
    int nbins, queue, defer;
    while (scanf("%d %d %d", &nbins, &queue, &defer) == 3)
        printf("%zu %zu\n", amof::tile_lds(nbins, queue, defer, false), amof::tile_lds(nbins, queue, defer, true));
    return 0;
}
