/* readback_page_check.c -- the bytes of readback_page.h's page, pinned.  The
 * read-back sims return before they build the page when there is no GPU, so
 * this program builds it for each damage profile and prints one line a
 * profile: the counts, and the scalar crc32c of the pristine and of the damaged
 * page.  tests/test_readback_page.py holds the lines.  No batch entry point is
 * called and no GPU is needed.
 */
#include "readback_page.h"

int main(void) {
    uint8_t *page = malloc(PAGE), *pristine = malloc(PAGE);
    if (!page || !pristine) return 1;
    crc32c_init();
    for (int profile = 0; profile < DAMAGE_PROFILES; ++profile) {
        struct page_counts c;
        if (page_build(page, pristine, profile, &c) != 0) return 1;
        printf("profile=%d nitems=%u live=%llu ndamaged=%llu nlen=%llu ndata=%llu nsame=%llu ntwo=%llu pristine=%08x "
               "damaged=%08x\n",
               profile, nitems, (unsigned long long)c.live, (unsigned long long)c.ndamaged, (unsigned long long)c.nlen,
               (unsigned long long)c.ndata, (unsigned long long)c.nsame, (unsigned long long)c.ntwo,
               crc32c(0, pristine, PAGE), crc32c(0, page, PAGE));
    }
    free(page);
    free(pristine);
    return 0;
}
