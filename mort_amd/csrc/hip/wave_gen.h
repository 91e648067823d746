/*
 * wave_gen.h -- launch interface of wave_gen.hip: MORT_MODE_WAVE (the queued / wavefront form of the render path) for
 * worlds without reference BVHs -- reference scenes 2..9, i.e. BASELINE config 5's book-2 final scene.
 */
#ifndef MORT_WAVE_GEN_H
#define MORT_WAVE_GEN_H

#include "mort_ctx.h"

/* Renders the owned rows through fronts of (path id, ray) records: wf_init_gen, then one wf_trav_gen + wf_shade_gen launch
 * pair per front until no pixel is live (wave_common.h wf_render).  a: the camera / partition / buffers; the unified-tree
 * image and constants come from c (as for mega_gen_kernel).  Fills `plan` with the traversal kernel it runs. */
int mort_wave_gen_render(mort_ctx *c, const mort_camera *cam, const RenderArgs &a, hipStream_t s, LaunchPlan &plan);

#endif
