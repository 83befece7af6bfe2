/*
 * host_sanitize_both_driver.c -- TEST INFRASTRUCTURE ONLY (tests/test_match_both_cpu.py).
 *
 * Drives the sgm_match_both family of the C host through the stand-in device (stub_device.c + stub_device_both.c) under
 * AddressSanitizer / UBSan: host forms (pageable), the pipelined form, the device form, batches, kept stages and their read-back,
 * a shape that grows, Q14, the post pass on its own stream, a refused launch in the middle of the both-views post pass.
 */
#include "../include/sgm_mi355x.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

void stub_fail_at(const char* name, int nth);
void stubb_set_pinned(int slot, const void* p);

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #x); return 1; } } while (0)

int main(void)
{
    SGMOption o;
    memset(&o, 0, sizeof o);
    o.num_paths = 8; o.min_disparity = 0; o.max_disparity = 16;
    o.is_check_lr = true; o.lrcheck_thres = 1.0f; o.is_check_unique = true; o.uniqueness_ratio = 0.99;
    o.is_remove_speckles = true; o.min_speckle_area = 50; o.p1 = 10; o.p2_init = 150;
    const int W = 64, H = 24, B = 2;
    const size_t big = (size_t)B * 2 * W * 2 * H;
    uint8_t* l = (uint8_t*)calloc(big, 1);
    uint8_t* r = (uint8_t*)calloc(big, 1);
    float* dl = (float*)calloc(big, sizeof(float));
    float* dr = (float*)calloc(big, sizeof(float));
    float* stage = (float*)calloc(big, sizeof(float));
    CHECK(l && r && dl && dr && stage);

    sgm_instance* s = sgm_create(0);
    CHECK(s && sgm_set_batch(s, B) && sgm_initialize(s, W, H, &o));
    CHECK(!sgm_match_both(s, l, r, dl, NULL) && !sgm_match_both(s, l, r, NULL, dr));
    CHECK(sgm_match_both(s, l, r, dl, dr));
    CHECK(dl[0] == 1.0f && dr[0] == 2.0f && dl[(size_t)B * W * H - 1] == 1.0f && dr[(size_t)B * W * H - 1] == 2.0f);
    CHECK(sgm_match_both(s, l, r, dl, dr));                                   /* Q14: no Reset */
    CHECK(sgm_reset(s, W, H, &o) && sgm_match_both_async(s, l, r, dl, dr) && sgm_match_both_async(s, l, r, dl, dr) && sgm_match_wait(s));
    CHECK(sgm_match_both_device(s, l, r, dl, dr) && sgm_synchronize(s));
    CHECK(sgm_match(s, l, r, dl) && sgm_match_both(s, l, r, dl, dr) && sgm_match(s, l, r, dl));
    sgm_keep_stages(s, 1);
    CHECK(sgm_reset(s, W, H, &o) && sgm_match_both(s, l, r, dl, dr));
    sgm_select_frame(s, B - 1);
    for (int which = 4; which <= 8; ++which) CHECK(sgm_read_stage(s, which, stage, big * sizeof(float)) == (size_t)W * H * sizeof(float));
    for (int which = 26; which <= 28; ++which) CHECK(sgm_read_stage(s, which, stage, big * sizeof(float)) == (size_t)W * H * sizeof(float));
    CHECK(sgm_match(s, l, r, dl) && sgm_read_stage(s, 28, stage, big * sizeof(float)) == 0);
    sgm_keep_stages(s, 0);
    /* a larger shape: every buffer of the instance goes and comes back */
    CHECK(sgm_reset(s, 2 * W, 2 * H, &o) && sgm_match_both(s, l, r, dl, dr) && dr[(size_t)B * 4 * W * H - 1] == 2.0f);
    CHECK(sgm_read_stage(s, 28, stage, big * sizeof(float)) == (size_t)4 * W * H * sizeof(float));
    CHECK(sgm_reset(s, W, H, &o) && sgm_match_both(s, l, r, dl, dr));
    /* page-locked outputs, both and one of the two; then pageable ones again */
    stubb_set_pinned(0, dl); stubb_set_pinned(1, dr);
    CHECK(sgm_reset(s, W, H, &o) && sgm_match_both(s, l, r, dl, dr) && dl[0] == 1.0f && dr[0] == 2.0f);
    stubb_set_pinned(0, NULL);
    CHECK(sgm_reset(s, W, H, &o) && sgm_match_both_async(s, l, r, dl, dr) && sgm_match_wait(s));
    stubb_set_pinned(0, dl); stubb_set_pinned(1, NULL);
    CHECK(sgm_reset(s, W, H, &o) && sgm_match_both_async(s, l, r, dl, dr) && sgm_match_both_async(s, l, r, dl, dr) && sgm_match_wait(s));
    stubb_set_pinned(0, NULL);
    /* the post pass on its own stream; then a launch refused inside the both-views post pass */
    CHECK(sgm_set_overlap_post(s, 1) && sgm_reset(s, W, H, &o));
    CHECK(sgm_match_both_async(s, l, r, dl, dr) && sgm_match_both_device(s, l, r, dl, dr) && sgm_synchronize(s));
    stub_fail_at("median", 0);
    CHECK(!sgm_match_both(s, l, r, dl, dr));
    CHECK(sgm_reset(s, W, H, &o) && sgm_match_both(s, l, r, dl, dr));
    CHECK(sgm_depth_from_both(s, dl, dr, (size_t)W * H, 1000.0f, 1001.0f, 100.0f, 0.0f, stage) && sgm_synchronize(s));
    sgm_destroy(s);

    /* the default instance */
    CHECK(!SGM_MatchBoth(l, r, dl, dr));
    CHECK(SGM_Initialize(W, H, &o) && SGM_MatchBoth(l, r, dl, dr) && dr[0] == 2.0f);
    SGM_Shutdown();
    free(l); free(r); free(dl); free(dr); free(stage);
    printf("host_sanitize_both_driver ok\n");
    return 0;
}
