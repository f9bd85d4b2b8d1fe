/*
 * fluidengine_ext.h — HIP-engine extensions, not part of the oracle ABI.
 *
 * include/fluidengine.h is the symbol set that the HIP library AND the two CPU oracle libraries export.  What only
 * fluidlab_amd/csrc/libfluidengine_hip.so has is declared here; a caller looks these names up on that library alone
 * (fluidlab_amd/_capi.py: EXT_SYMBOLS).  Conventions are those of fluidengine.h: 0 on success, fe_last_error() otherwise.
 *
 * Material-parameter gradients
 * ----------------------------
 * d loss / d mu[p], d loss / d lam[p], d loss / d rho[p] for the per-particle values given to fe_init_particles.  The
 * reference has no counterpart: its mu, lam and rho fields carry no needs_grad (mpm_simulator.py:73-135).
 *
 *   fe_set_option(h, "param_grad", 1)   turns the pass on: every backward substep (fe_substep_grad, fe_step_grad) then adds its
 *                                       contribution to three fp64 accumulators of N entries each, by particle id.  They are allocated
 *                                       and zeroed the first time the option is set.  fe_get_option reports it.  Refused for scenes
 *                                       with MAT_RIGID particles (their density also enters the shape-matching centre of mass);
 *                                       fe_step_grad_batch refuses engines that have it on (no batched form).
 *   fe_reset_grad(h)                    also zeroes the accumulators (like every other adjoint); fe_reset_grad_till_frame does not.
 *
 * A sweep accumulates: after fe_reset_grad, seeding the loss adjoints and the fe_step_grad calls back to frame 0, the
 * accumulators hold the derivative of the loss over all substeps of the sweep.  Out of scope: batched environments, MAT_RIGID
 * bodies, derivatives with respect to p_vol, dt, gravity, the yield bounds or collider friction.
 *
 * Frame reads that stay on the GPU: observation gather and frame summary
 * -----------------------------------------------------------------------
 * Two everyday reads of a frame without copying it to the host (fe_get_frame moves 28 N bytes for x, v and used alone).  The
 * reference's counterparts are host code over downloaded fields (fluid_env.py:102-129 picks ~200 particles per body out of
 * get_state_RL; its only health check is np.isnan(reward), fluid_env.py:94).
 *
 *   fe_obs_set_particles   a list of particle ids; fe_obs_get / fe_obs_get_dev then return the rows of exactly those particles of any frame,
 *                          found through the slot_of_pid of the frame's own particle order: n rows cross PCIe, not N.
 *   fe_summary_set_groups  assigns every particle id to one of up to FE_SUMMARY_MAX_GROUPS groups (bodies, materials, ...) or to none (-1).
 *   fe_frame_summary       one FeFrameSummary per group plus one for the whole frame, reduced on the device in fp64.
 *
 * Contract
 *   - f is a local frame index, checked like fe_get_frame's.  Every call enqueues on the engine's stream and returns after it has drained.
 *   - Read-only: no frame, order table, sort key or dirty flag changes and a compactly stored F is NOT expanded (it is read as c I).  A rollout
 *     with these calls in it launches the same substep kernels, and computes the same frames, as one without.
 *   - m is the fp32 mass the engine holds (p_vol * rho, rounded to fp32 by fe_init_particles).  Every product and sum is formed in fp64 from the
 *     fp32 words; J = det F is the cofactor expansion along the first row in fp64.  No fp32 accumulation, no floating-point atomics: the
 *     result does not depend on timing, only -- within fp64 rounding of the sums -- on the particle order of the frame.
 *   - Unused particles (used == 0, the Injector's pool parked at NOWHERE included) contribute nothing anywhere.  A used particle with a
 *     non-finite word in x, v, C or F is counted in n_used and n_nonfinite and contributes to nothing else.
 *   - A group that is empty, or whose used particles are all non-finite, gives zeros apart from the two counts.
 *   - Errors (0 otherwise): no observation list, a particle or group id out of range (list / groups unchanged), a wrong record_size.
 *   - Engines stepped through fe_step_batch take the calls one by one between batch calls.  fe_destroy frees the buffers.
 * Out of scope: batched forms, angular momentum, adjoints of any of these quantities.  The smoke field has its own reads (below).
 *
 * Task losses in the engine: loss-term programs
 * ---------------------------------------------
 * The task losses of GatheringEasy, GatheringO, Pouring, Transporting and Mixing (the reference's fluidlab/fluidengine/losses) are sums over
 * particle positions: L1 / squared distance to a constant, L1 distance to a remembered frame, L1 distance over all pairs of two sets.  Such a
 * loss is registered once as a list of at most FE_TASK_LOSS_MAX_TERMS terms (fe_task_loss_set_terms); one call per step then evaluates the
 * program on a GPU-resident frame (fe_task_loss_step) or adds its gradient to the frame's adjoint (fe_task_loss_step_grad).
 *
 * Term values (sel = selected by `a`, sums over the axes in axis_mask, w = weight):
 *   FE_TERM_L1_CONST   w * sum_{p in sel} sum_axes |x_pa - c_a|
 *   FE_TERM_SQ_CONST   w * sum_{p in sel} sum_axes (x_pa - c_a)^2
 *   FE_TERM_L1_REF     w * sum_{p in sel} sum_axes |x_pa - ref_pa|          (ref: fe_task_loss_set_ref)
 *   FE_TERM_PAIR_L1    w * sum_{i in a, j in b} sum_axes |x_ia - x_ja|;  with b.pid_lo < 0 the same over all ORDERED pairs (i, j) of a
 *                      with itself (every unordered pair twice: what mixing_loss.py:72-75 sums)
 * d|d| is sign(d), 0 at d == 0: ties and i == j contribute nothing.  A pair gradient is w times an integer count: for a_i across two sets
 * #{b < a_i} - #{b > a_i} per axis, for b_j the mirrored count, for self pairs twice the count.
 *
 * Contract
 *   - Precision: every difference, product and sum is formed in fp64 from the fp32 position words.
 *   - Determinism: no floating-point atomics; partial sums are merged in a fixed order.  Pair counts use integer atomics when a set is
 *     split over several chunks (option "task_pair_chunk": rows of the other set per workgroup, a multiple of 64; 0 = chosen by the engine),
 *     and integer addition does not depend on order: two evaluations of a frame give bit-identical step_loss and adjoints.
 *   - Gradient rounding: per particle and axis the gradient of all terms (pair counts included) is summed in fp64 in term order, multiplied
 *     by scale, rounded to fp32 ONCE and added to the adjoint with one read-modify-write.
 *   - fe_task_loss_step_grad handles an adjoint slot stored in another particle order than the frame (like fe_loss_step_grad) and refuses
 *     a frame whose adjoint a fused fe_step_grad passed on in registers, with the same error.
 *   - fe_task_loss_step only reads the frame: no table, sort key or dirty flag changes, a compactly stored F stays compact, a rollout
 *     with these calls in it launches the same substep kernels and produces the same frames.
 *   - Neither step call waits for the stream; only fe_task_loss_get does.
 *   - Errors (non-zero, fe_last_error, the previous program stays): an unknown kind or an empty axis_mask, a pid range outside [0, N],
 *     more than FE_TASK_LOSS_MAX_TERMS terms or FE_TASK_LOSS_MAX_PAIR_TERMS pair terms, a wrong term_size, two-set pair terms whose pid
 *     ranges overlap; at a step: FE_TERM_L1_REF before fe_task_loss_set_ref, s outside the allocated steps, no program set.
 *   - Nothing is allocated before fe_task_loss_alloc / fe_task_loss_set_terms; fe_destroy frees everything.
 * Out of scope: batched forms, gradients with respect to c, weight or ref, and the Pouring 'diff'
 * attraction term (argmin plus the 100 nearest particles), which stays with its caller.  The smoke field's CirculationLoss is fe_smoke_loss_* (below).
 *
 * Density fields: shape targets without a recorded trajectory
 * -----------------------------------------------------------
 * A field is a box of n[0] x n[1] x n[2] cells (FeDensitySpec); cell (i, j, k) has linear index (i n[1] + j) n[2] + k and centre
 * origin + (i + 0.5, j + 0.5, k + 0.5) cell.  A particle deposits the product over the axes of quadratic B-spline weights: with
 * u = (x_a - origin_a) / cell_a, s = u - 0.5, b = floor(s - 0.5), t = s - b in [0.5, 1.5) the cells b, b + 1, b + 2 get 0.5 (1.5 - t)^2,
 * 0.75 - (t - 1)^2 and 0.5 (t - 0.5)^2 (derivatives -(1.5 - t) / cell_a, -2 (t - 1) / cell_a, (t - 0.5) / cell_a).  An axis with n[a] == 1
 * is projected: weight 1, derivative 0, wherever the particle is.  Stencil cells outside [0, n) are dropped, in value and in gradient.  A
 * particle with a non-finite position word, or with |u| > 2^30 on an unprojected axis, deposits nothing and gets no gradient.
 *
 *   fe_density_set_field    defines (or, with spec == NULL, removes) one of FE_DENSITY_MAX_FIELDS fields; drops the field's target
 *   fe_density_set_target   the field's target T, one fp64 value per cell, copied to the device
 *   fe_density_get          D of frame f for a selection of particles, to the host: a top-down image of a material when y is projected
 *   FE_TERM_DENSITY_SQ      a term of a loss-term program: w * sum_c (D_c - T_c)^2 over the particles selected by `a`, with the gradient
 *                           d / d x_pa = w * sum_c 2 (D_c - T_c) d w_pc / d x_a.  axis_mask must be 7; the field id travels in b.pid_lo and the
 *                           rest of b is zero.  At most FE_TASK_LOSS_MAX_DENSITY_TERMS density terms per program.
 *
 * Contract
 *   - Fixed point: each deposit is q = llrint(w 2^40), added to an unsigned 64-bit cell word; D_c = (double)word / 2^40.  Integer addition
 *     does not depend on order, so a field is the same bits however it was accumulated: in per-workgroup LDS copies flushed with integer
 *     atomics (fields of at most 8192 cells) or straight with 64-bit integer global atomics.  Option "density_lds": -1 the engine chooses,
 *     0 never the LDS road, 1 whenever the field fits.  No floating-point atomics anywhere.
 *   - Engines with N > 2^23 are refused, so that no cell word can overflow; fields have at most FE_DENSITY_MAX_CELLS cells.
 *   - The task-loss contract above holds for the density term: the calls only read the frame; the step calls do not wait for the stream
 *     (fe_density_get does); fe_task_loss_step_grad recomputes the field of frame f; per particle and axis the gradients of all terms are
 *     summed in fp64 in term order, multiplied by scale and rounded to fp32 once; an adjoint stored in another particle order is handled and
 *     one passed on in registers is refused.
 *   - Errors (non-zero, fe_last_error, the previous program, field or target stays): a field id out of range, a wrong spec_size, n[a] < 1,
 *     more than FE_DENSITY_MAX_CELLS cells, a cell size or origin that is not finite (cell: and positive), an n_cells that does not match the
 *     field, N > 2^23; at fe_task_loss_set_terms a density term that names a field that is not set; at a step a density term whose field has
 *     no target.
 * Out of scope: batched forms, per-step targets, gradients with respect to the target or the spec, colour or rendering.
 *
 * Target clouds and the Chamfer terms: nearest-neighbour shape targets
 * ------------------------------------------------------------------
 * The density term's gradient is local: a target that does not overlap the fluid pulls on nothing.  A cloud is a set of up to
 * FE_CLOUD_MAX_POINTS target points without correspondence to particle ids (fe_cloud_set, FE_CLOUD_MAX of them); two term kinds measure a
 * frame against it (sel = selected by `a`, m = axis_mask as a 0/1 vector, w = weight; the cloud id travels in b.pid_lo, the rest of b is 0):
 *   FE_TERM_NEAREST_SQ   w * sum_{p in sel}   min_j |m.(x_p - t_j)|^2          each selected particle to its nearest cloud point
 *   FE_TERM_COVER_SQ     w * sum_{j in cloud} min_{p in sel} |m.(t_j - x_p)|^2 each cloud point to its nearest selected particle
 * A Chamfer loss is one term of each kind.  Any non-empty mask is legal: axes outside it count as 0 in the search and in the distance and get
 * no gradient (x | z: the match seen from above).  At most FE_TASK_LOSS_MAX_NEAREST_TERMS such terms per program.  Gradients:
 *   NEAREST  d / d x_pa = w * 2 m_a (x_pa - t_{j*(p),a}),  j*(p) the nearest cloud point of p
 *   COVER    d / d x_pa = w * 2 m_a sum_{j: p*(j) = p} (x_pa - t_ja),  p*(j) the nearest selected particle of point j
 * fe_cloud_query returns j*, p* and both d2 arrays to the host.
 *
 * Contract
 *   - Arithmetic: d_a = (double)x_a - (double)t_a; d2 = (d_x d_x + d_y d_y) + d_z d_z in fp64, in that order, without fused multiply-add (fp
 *     contraction is off in fe_nn_d2); a masked axis contributes 0 * 0.  A brute-force numpy restatement reproduces d2 bit for bit.
 *   - Ties: the nearest is the smallest d2; among equal d2 the lowest cloud index (NEAREST) or the lowest particle id (COVER) wins.  The
 *     result is a function of the frame's contents only: not of the particle order, the search structure or timing.
 *   - Skipped points: a particle with a non-finite position word, or with |x_a| > FE_CLOUD_COORD_MAX on an axis of the mask, is neither a
 *     query nor a candidate and gets no gradient.  fe_cloud_set refuses a point with such a coordinate on any axis.
 *   - Empty sets: with no candidate particle COVER's value is 0 and nn_of_point is -1.  Clouds are never empty.
 *   - Values: the d2 of the queries are summed in fp64 in the fixed-order scheme of the other terms -- workgroup partials chunked by query
 *     index (pid or cloud index, whatever the frame's particle order), then the fixed-order merge.  Two evaluations of a frame give the same
 *     bits; the value lies within (n - 1) 2^-53 sum d2 of any other fp64 summation of the n values.
 *   - COVER's gradient without floating-point atomics: each cloud point adds llrint(d_a 2^40) to three signed 64-bit words of its nearest
 *     particle with integer atomics (|d_a| <= 4 and n <= 2^20, so |sum| <= 2^62: no overflow); the adjoint kernel turns the words back into
 *     fp64.  Integer addition does not depend on order, so the bits repeat; a particle's sum lies within c_p 2^-41 of the fp64 sum, c_p the
 *     number of points that chose it.
 *   - The search: a uniform grid over the bounding box of the indexed set (a reduction), masked axes collapsed to one cell; counts per cell
 *     with integer atomics, an exclusive scan, a fill into a compact (x, y, z, id) array.  A query's cell is clamped into the grid and the
 *     Chebyshev rings r = 0, 1, ... of cells around it are searched until best_d2 <= (r h_min)^2 + gap^2 (h_min: the smallest cell edge over
 *     the unmasked axes with more than one cell; gap: the distance from the query to the box, 0 inside it, so that a query far from the set
 *     does not walk the whole grid; the sum taken 2e-6 short for the rounding of the cell index) or the ring has left the grid on every side.
 *     A cloud's index is built once per (cloud, mask) -- at fe_task_loss_set_terms or the first query, and again when "nn_cells" changed --
 *     the particles' index per call.  Option "nn_cells": 0 = the engine chooses the resolution (about four points per cell, at most 64 cells
 *     along an axis), k > 0 = at most k cells along the longest axis, k = 1 = brute force through the same kernel.  Every setting gives the
 *     same bits in every output.
 *   - The task-loss contract above holds: per particle and axis the gradients of all terms are summed in fp64 in term order, multiplied by
 *     scale, rounded to fp32 once and added with one read-modify-write; an adjoint stored in another particle order is handled, one passed on
 *     in registers is refused; the step calls only read the frame and do not wait for the stream (fe_cloud_query does);
 *     fe_task_loss_step_grad rebuilds what it needs from frame f.
 *   - Errors (non-zero, fe_last_error, the previous program and cloud stay): a cloud id out of range, n > FE_CLOUD_MAX_POINTS, a refused
 *     coordinate, removing a cloud that the current program names; at fe_task_loss_set_terms a term that names a cloud that is not set, a
 *     non-zero rest of b, more than FE_TASK_LOSS_MAX_NEAREST_TERMS nearest terms.
 * Out of scope: batched forms, gradients with respect to the cloud, per-step clouds, k > 1 neighbours (Pouring's attraction term stays with
 * its caller).
 *
 * Smoke-field reads that stay on the GPU: cell lists, detector loss, field summary
 * --------------------------------------------------------------------------------
 * The smoke-side counterpart of fe_obs_*, fe_task_loss_* and fe_frame_summary.  fe_smoke_get_frame moves whole fields (a 128^3 scalar is
 * 8.4 MB); Circulation-v0 reads 1,352 lattice cells for its observation and fifteen detector cells for its loss (the reference's
 * circulation_env.py / circulation_loss.py index downloaded fields), and its only health check is np.isnan(reward).
 *
 *   fe_smoke_cells_set        one of FE_SMOKE_MAX_LISTS lists of cells (i, j, k); fe_smoke_cells_get / _get_dev then return v and q of exactly
 *                             those cells of any frame, gathered into one staging buffer: n (3 + q_dim) words cross PCIe in one copy.
 *   fe_smoke_loss_*           sum_i w_i |q[s, cell_i, comp] - t_i| (FE_SMOKE_SQ: squared) over a list, added to step_loss[s_loss]; its gradient added
 *                             to the q adjoint.  The detectors are the list's cells as they were at fe_smoke_loss_set: changing or removing the
 *                             list afterwards does not change the loss.
 *   fe_smoke_summary          one FeSmokeSummary of frame s, reduced on the device in fp64.
 *   fe_smoke_cells_add_grad   the adjoint of fe_smoke_cells_get: n cotangent rows scattered into the v / q adjoint of frame s at the list's cells
 *                             (a closed-loop policy that observes the field: n (3 + q_dim) words instead of two dense fields).
 *
 * Contract
 *   - Frames: s is a local smoke frame in [0, max_steps_local], checked like fe_smoke_get_frame's; s_loss indexes the allocated loss steps.
 *   - Stream: every call enqueues on the engine's stream; only fe_smoke_cells_get, fe_smoke_cells_add_grad, fe_smoke_loss_get
 *     and fe_smoke_summary wait for it.
 *   - Read-only: the reads and fe_smoke_loss_step change no field, mask or adjoint; a rollout with these calls in it computes the same smoke
 *     frames, bit for bit, as one without.  fe_smoke_loss_step_grad adds to gq and to nothing else.
 *   - Cell lists: cells are checked against res when the list is set; on error the list is left unchanged.  Duplicates are allowed in a list
 *     that is only read; fe_smoke_loss_set refuses a list with a duplicate cell (each gradient entry is one read-modify-write, there are no
 *     floating-point atomics).  fe_smoke_create drops every list, the loss and its buffers; fe_destroy frees them.  Nothing is allocated
 *     before the first _set or _alloc.
 *   - Cell-list adjoint: fe_smoke_cells_add_grad* change gv[s] and gq[s] at the listed cells and nothing else -- no field, mask, other frame
 *     or other adjoint.  Duplicates in the list are legal: the rows of one cell are summed in list order in fp32, starting from 0, and the
 *     sum is added to the adjoint word once, by the one thread that owns the cell.  No floating-point atomics; the result does not depend on
 *     launch geometry or timing and equals, bit for bit, what fe_smoke_add_grad adds for a host field accumulated row by row, in list order,
 *     on an fp32 zero field.  The rows are grouped once per list at the list's first use (row indices stably sorted by linear cell index,
 *     plus segment starts); fe_smoke_cells_set on that list drops the grouping.  The host variant stages through the engine and returns
 *     after the stream has drained; the _dev variant enqueues and does not wait, like fe_smoke_cells_get_dev: gv and gq stay as they are
 *     until the engine's stream has passed.  Nothing is allocated before the first call.
 *   - Loss value: every difference, product and sum is formed in fp64 from the fp32 words.  Partial sums are merged in a fixed order (thread t
 *     of 256 adds the entries t, t + 256, ...; the butterfly of fe_task_loss.h within a wave; the four waves in order): two evaluations of
 *     a frame give the same bits, and the value lies within (n - 1) 2^-53 sum |terms| of any other fp64 summation.  d|d| is sign(d), 0 at d == 0.
 *   - Loss gradient: rounded to fp32 once, (float)(scale * w_i * sign(d_i)) (FE_SMOKE_SQ: 2 d_i for sign(d_i)), and added to gq with one
 *     read-modify-write: the bits the dense road adds (a host field of these values through fe_smoke_add_grad).  A non-finite q at a detector
 *     makes the value non-finite and adds no gradient there.
 *   - Summary: covers the slab cells lower_y < j < higher_y, all i and k, of frame s.  It reads v and q only -- not the free mask, v_tmp, div
 *     or p, which belong to the step and not to the state.  A cell with a non-finite word in v or q counts in n_nonfinite and contributes to
 *     nothing else.  v_max = max |v_a| over cells and axes; courant = dt * v_max (v is in cells per unit time: the back-trace subtracts
 *     dt v from positions in cell units); kinetic = 1/2 sum |v|^2; q_sum, q_min, q_max per component, entries beyond q_dim zero.  Sums are
 *     fp64 in a fixed order over workgroup partials, extremes are comparisons of widened fp32 words.  An empty slab, or one in which every
 *     cell is non-finite, gives zeros apart from the two counts.
 *   - Errors (non-zero, fe_last_error, the previous state stays): no smoke field; a list id out of range or a list not set; a cell out of
 *     range; n above FE_SMOKE_MAX_LIST_CELLS; comp outside [0, q_dim); an unknown kind; a wrong record_size; a step before
 *     fe_smoke_loss_alloc or fe_smoke_loss_set; s_loss outside the allocation.
 * Out of scope: batched environments, gradients with respect to targets or weights, residual divergence, colour or rendering, any change
 * to the solver itself.
 *
 * Headless particle renderer: a picture of a GPU-resident frame
 * -------------------------------------------------------------
 * The reference draws every moving thing as spheres with a colour per vertex (GGUIRenderer.render_frame: particles, target particles,
 * smoke markers).  Here that is a scatter over a frame: every used particle, and every point of up to FE_RENDER_MAX_SETS static point
 * sets, is a sphere; per pixel the nearest fragment wins through a 64-bit integer atomicMin; one more pass shades the winners.
 *
 *   fe_render_setup       camera, lights and the image buffers (calling it again re-sizes them)
 *   fe_render_set_colors  RGBA8 per particle id and the particles' world radius
 *   fe_render_set_points  a static point set (target particles, markers): ids N + set * FE_RENDER_MAX_POINTS + i
 *   fe_render_frame       clear + splats + shade of frame f, enqueued
 *   fe_render_get / _dev  RGBA8 [H][W][4], depth fp32 [H][W] (+inf on background), id int32 [H][W] (-1 on background)
 *
 * Geometry (all in fp64 from the fp32 position words, + - * / and sqrt only, no contraction: the host build of fe_render.h, the device
 * and a restatement in another language that performs the same operations in the same order give the same bits)
 *   - Camera: pos, an orthonormal right / up / fwd, focal in pixels (0.5 H / tan(fov_y / 2)), computed by the caller; no trigonometry here.
 *   - A sphere of centre x, world radius R: d = x - pos, zc = d.fwd, xc = d.right, yc = d.up.  Dropped if a word of x is non-finite or
 *     unless zc > near + R.  px = W/2 + focal xc / zc, py = H/2 - focal yc / zc, rp = min(focal R / zc, max_radius_px).
 *   - Its box: columns floor(px - rp - 0.5) .. ceil(px + rp - 0.5), rows likewise, clipped to the image.
 *   - A fragment at pixel (i, j) of the box: u = (i + 0.5 - px) / rp, v = (j + 0.5 - py) / rp, s = u^2 + v^2; covered when s <= 1.  The pixel
 *     that contains (px, py) is always covered, with s clamped to 1: a sub-pixel sphere never vanishes.  nz = sqrt(1 - s),
 *     depth = (float)(zc - R nz).
 *   - The pixel word is (bits of depth << 32) | id; the smallest word wins: the nearest fragment, the lowest id among equal depths.  The id
 *     is the particle id, never the slot: a frame stored in another particle order gives the same image.  Background: all ones.
 *   - Shade: n = u right - v up - nz fwd of the winning sphere, surface point x + R n, colour = base (ambient + sum over the lights of
 *     light_colour max(0, n.l)) with l the unit vector from the surface point to the light, clamped to [0, 1], byte = (int)(c 255 + 0.5),
 *     alpha 255.  A background pixel gets the background colour.
 *
 * Contract
 *   - Read-only: no frame, table, sort key or dirty flag changes and a compactly stored F stays compact; a rollout with render calls in it
 *     computes the same frames bit for bit.  Unused particles (the Injector's parked pool included) are not drawn.
 *   - Deterministic: integer atomics only; two renders of a frame give the same bytes.  A sphere whose clipped box has more than
 *     "render_lane_pixels" pixels (fe_set_option; default FE_RENDER_LANE_PIXELS) is drawn by the 64 lanes of its wave together, a smaller
 *     one by its own lane; both roads produce the same words.
 *   - fe_render_frame and fe_render_get_dev do not wait for the stream; fe_render_get does.
 *   - Nothing is allocated before fe_render_setup; fe_destroy frees everything.
 *   - Errors (non-zero, fe_last_error, the previous state stays): a wrong struct size; width or height outside [1, 4096]; a focal, near,
 *     radius or max_radius_px that is not finite and positive; a position, basis, light or colour that is not finite; more than
 *     FE_RENDER_MAX_LIGHTS lights; a set index out of range; n above FE_RENDER_MAX_POINTS; any call before fe_render_setup; fe_render_frame
 *     before fe_render_set_colors; fe_render_get before fe_render_frame; a frame index fe_get_frame would refuse.
 * Out of scope: triangle meshes (colliders are drawn from their SDFs, below), shadows, transparency of anything but a liquid (drawn as a
 * translucent surface by fe_surface_*, below), anti-aliasing, batched engines, a window
 * (mode='human'), gradients through the image.
 *
 * The scene in that picture: SDF colliders ("volumes") and the smoke field
 * ------------------------------------------------------------------------
 * The reference also draws the meshes of statics and effectors and one sphere per cell of the smoke field (GGUIRenderer.render_frame,
 * SmokeField's vis_particles).  There are no mesh assets here; the engine holds every collider as the SDF block it collides with, and those
 * are drawn where they lie, into the same pixel words, composited by the same integer atomicMin.  Off until asked for.
 *
 *   fe_render_set_volume   slot c of FE_RENDER_MAX_VOLUMES: engine static i, the mesh of effector e (posed by its position and quaternion
 *                          words of the frame drawn, read on the device), or the renderer's own copy of an FeSdfDesc + voxels (a visual-only
 *                          static the engine never receives); an RGBA8 colour; id N + FE_RENDER_MAX_SETS * FE_RENDER_MAX_POINTS + c
 *   fe_render_set_scene    march_step, bisect_iters; draw_smoke, the visible slab lo < j < hi, the cells' radius, the cold and hot colours
 *   fe_render_scene_frame  what fe_render_frame(f) enqueues, then k_render_smoke (smoke frame s, when smoke is on), k_render_sdf (when a
 *                          volume is set), k_render_shade_scene.  With no scene and no volume: exactly fe_render_frame.  s is ignored
 *                          without smoke.  fe_render_get / _dev return its buffers as they return fe_render_frame's.
 *
 * Geometry (the rules above: fp64 from fp32 words, + - * / sqrt, no contraction)
 *   - The ray of pixel (i, j): P(t) = pos + t d, d = fwd + ((i + 0.5 - W/2) / focal) right - ((j + 0.5 - H/2) / focal) up.  d is not normalised:
 *     t is the depth along fwd, the quantity the sphere fragments store.
 *   - A volume: the ray is mapped into voxel coordinates (for an effector first the inverse pose: rotate pos - p and d by the conjugate of the
 *     normalised quaternion, as t_dynamic_collide does; then rows 0..2 of T), where it is linear in t: pv(t) = ov + t dv.  It is clipped against
 *     [0, res - 1]^3 by the slab test and against t >= near, giving [t0, t1].  Sample k lies at t0 + k dt with dt = march_step / |dv| (computed
 *     so, not accumulated), k = 0 .. min(floor((t1 - t0) / dt), 4096).  A sample is the trilinear sample of t_sdf_sample in its order of
 *     operations (1 outside the box).  The first sample with sd <= 0 is a hit: at t0 when k == 0 (the camera is inside, or the solid reaches the
 *     box's face); otherwise the bracket [t_(k-1), t_k] is bisected bisect_iters times (mid = 0.5 (lo + hi); sd(mid) <= 0 moves the upper end,
 *     else the lower) and the hit is the upper end.  The fragment is (bits of (float)t_hit << 32) | id, kept when smaller than the pixel's word.
 *     Only the SIGN of the SDF is used -- the stand-in SDFs are scaled, so sphere tracing by value would be wrong.  A wall thinner than the
 *     march step can be missed.  The kernel may stop a march early where that cannot change the word (behind the pixel's current depth).
 *   - Smoke: every cell (i, j, k) of the slab, free or not (the walls win by depth), is a sphere with the fp32 centre words
 *     ((float)c + 0.5f) * (1.f / (float)n) and the scene's radius, drawn like a point set (both roads), id N + FE_RENDER_MAX_SETS *
 *     FE_RENDER_MAX_POINTS + FE_RENDER_MAX_VOLUMES + (i n + j) n + k.
 *   - Shade, cell: base = byte(cold (1 - q) + hot q) per channel with q = (double)q[s][cell][0] (a non-finite q gives 0 through the byte
 *     rule); then as a particle.  Shade, volume: hit point P = pos + (double)depth d from the stored fp32 depth (no second march); normal =
 *     central differences of the SDF at pv((double)depth) with delta = 1e-2 voxels, each divided by 2 delta, times Rinv, rotated by the
 *     normalised pose quaternion for an effector, divided by its length (a vanishing or non-finite length: -fwd), negated when n.d > 0; colour
 *     = base (ambient + sum light_colour max(0, n.l)), l the unit vector from P to the light, as for a sphere.
 *
 * Contract
 *   - Read-only and deterministic like the particle picture; the four kernels of fe_render_frame and its launches are untouched.
 *   - A statics' or effector's slot holds the parameter block as it was when the slot was set; the voxels are the engine's own.
 *   - Own copies are allocated by fe_render_set_volume and freed when the slot is set again or cleared, and by fe_destroy.
 *   - Errors (non-zero, fe_last_error, the previous state stays, the next picture is the one it would have been): any call before
 *     fe_render_setup; a slot, static or effector index out of range; an effector without a mesh; an unknown source or a null colour; a wrong
 *     struct size; a march_step or smoke radius that is not finite and positive, or a march_step above 1; bisect_iters outside [0, 32];
 *     draw_smoke without a smoke field; a slab outside the grid; a grid whose largest cell id would not fit a positive int; s outside
 *     [0, max_steps_local] while smoke is on; whatever fe_render_frame refuses.
 * Out of scope: transparency of a collider (one with alpha < 1 is the caller's to skip; liquids have fe_surface_*, below), shadows,
 * anti-aliasing, triangle meshes, a window.
 *
 * Contact wrenches: what every collider's contact law did, per substep
 * --------------------------------------------------------------------
 * The engine applies a contact law at its SDF colliders in every substep -- agent.collide on the gathered particle velocity (mpm:418-422) and
 * the collider chain inside grid_op (mpm:386-395: the statics, then the effectors when collide_type has bit 1) -- and differentiates through
 * it, but the reference has no call that says what the contact did.  fe_contact_wrench replays both chains of substeps f0 .. f0 + n - 1 from what
 * the forward pass left on the device (the frame's stored grid, its contact flags) and returns, per collider, the linear and angular impulse the
 * collider gave to the material.  The colliders are the effectors 0 .. n_eff - 1, then the statics in the order of fe_add_static.
 *
 *   particle part   for every used particle of frame f whose contact flag g2p set: nv = the 27-node B-spline sum of v_out of frame f (fp32, read
 *                   from the frame's grid store through the frame's own order table); the effectors that carry a mesh in order, pos = x + dt nv
 *                   re-formed before each, skipped while pos_y <= collide_min_y.  Where the collider takes its contact branch:
 *                   dv = v_after - v_before per axis in fp64 from the fp32 words, J = (double)m dv, r = the fp32 pos the collider saw;
 *                   impulse += J, ang_impulse += r x J, n_particles += 1.
 *   node part       for every stored node with mass m > 1e-12: v = dt g + p / m as grid_op forms it (fp32), the statics in order, then the
 *                   effectors when the engine collides at nodes; the same dv and J = (double)m dv per collider that took its contact branch, r =
 *                   the node's position; n_nodes += 1.  The domain boundary's own change belongs to no collider and is not reported.
 *
 * Contract
 *   - Read-only: no frame, table, sort key, stamp, dirty mark, working grid or store word changes and a compactly stored F stays compact.  A
 *     rollout with these calls in it launches the same substep kernels and computes the same frames bit for bit.
 *   - Only from the store: a frame whose grid is not in the store gives valid = 0 and zeros -- option grid_store = 0, a frame with a slow-path
 *     particle or more active blocks than the store has slots (its flag is 0), a frame fe_set_frame has written since.  Nothing is recomputed.
 *   - Which frames: the replay reads the frame's store record through the order table the frame has NOW and the effectors' pose words as they
 *     are NOW.  Only fe_set_frame clears a frame's store flag.  So the records describe what the forward pass did for the frames of the current
 *     window whose effector poses have not been written since (fe_eff_set_state on a frame already computed, a frame index left over from an
 *     earlier sweep whose table has been rebuilt: valid may still be 1 and the values mean nothing; the reads stay inside the frame's record).
 *   - Precision: everything the contact law computes is the engine's fp32, in its order of operations, so that the replay takes the branches the
 *     forward pass took (the particle gather may sum its 27 products in another order than g2p: a particle within rounding of a surface can
 *     fall on the other side).  fp64 is used for the products m dv, r x J and the sums only.
 *   - Deterministic: no floating-point atomics; per-lane sums in slot / entry order, the butterfly of fe_task_loss.h within a wave, the waves
 *     of a workgroup in order, the workgroups' partial records in index order.  Two evaluations of a frame give the same bits; the result
 *     depends on the frame's particle order only through fp64 rounding of the sums.
 *   - MAT_RIGID particles are counted as the contact law moved them, before the rigid-body pass overrides their velocities.  Unused particles
 *     contribute nothing.  A non-finite word makes the record non-finite, and that is what is reported.
 *   - Sign: the impulses are the material's.  Force and torque ON the collider are -impulse / dt and -ang_impulse / dt; the call does not divide.
 *     ang_impulse is taken about the world origin; about the effector it is ang_impulse - ref x impulse.
 *   - An effector without a mesh gives zeros, with the frame's valid.
 *   - Errors (non-zero, fe_last_error, `out` untouched): f0 < 0, n < 1, f0 + n > max_substeps_local, a wrong record_size, n_records < 1, a
 *     null `out`; a null handle returns non-zero.  An engine without colliders has fe_contact_count() == 0 and the call succeeds writing nothing.
 *   - One set of launches per substep on the engine's stream, then one copy and one wait.  Nothing is allocated before the first call;
 *     fe_destroy frees the partial and output buffers.
 * Out of scope: batched forms (engines of a batch take the call one by one between batch calls), adjoints of the wrench and loss terms on
 * it, the boundary's impulse, per-particle or per-node contact maps, making more frames storable.
 *
 * Liquids in that picture: one smoothed, translucent screen-space surface
 * -----------------------------------------------------------------------
 * The reference's GL renderer marks every body whose material class is MAT_LIQUID as one that "needs smoothing" (gl_renderer.py:71-105) and draws
 * it as one surface one can look into, not as a pile of beads.  Here the selected particles leave the opaque picture and become a second layer:
 * nearest fragment and summed thickness per pixel, a depth-aware smoothing of the layer's depth, a normal from the smoothed depth, one lit colour
 * blended over the opaque picture by the thickness.  Off until asked for; with it off every picture is the bytes it was.
 *
 *   fe_surface_set        sel[N] by particle id (0 = opaque) and a FeSurfaceParams.  A null or all-zero sel switches the surface off.
 *   fe_surface_frame      what fe_render_scene_frame(f, s) enqueues, with the surface; enqueued, no wait.  With the surface off it is exactly
 *                         fe_render_scene_frame.  fe_render_get / _dev return the finished picture (rgba, depth, id) as they always do.
 *   fe_surface_get / _dev the layer's own images of the last fe_surface_frame, [H][W] each, any may be null: z_raw (fp32 depth of the nearest
 *                         liquid fragment, +inf where there is none), z_smooth (after the passes), thickness (fp64, world length)
 *
 * FeSurfaceParams: radius_scale >= 1 (liquid spheres are drawn with R_s = radius_scale R); smooth_iters in [0, 8] passes; smooth_radius_px r in
 * [1, 8]; range > 0 in depth units (neighbours further apart are not blended); absorb >= 0 per unit length; alpha_min in [0, 1], the lower
 * bound of the liquid's opacity; specular in [0, 1], the weight of the highlight; shininess_log2 k in [0, 10]: the highlight is raised to 2^k.
 *
 * Numeric rules (the renderer's, stated once): fp64 formed from fp32 words; only + - * / and sqrt; fp contract(off); no exp or pow -- the
 * highlight is max(0, n.h) squared k times; integer atomics only; the per-pixel math is __host__ __device__ code (fe_surface.h) that a host
 * program compiles and a restatement in another language repeats operation for operation.
 *   1 Opaque layer.  Everything but the selected particles -- unselected used particles, point sets, and with a scene the smoke cells and
 *     volumes -- is drawn and shaded as fe_render_scene_frame draws it, by the same kernels; only the particle splat is replaced by one that
 *     skips the selected ids and calls the same code for the others.
 *   2 Liquid layer.  After 1 has finished: every selected used particle, projected with R_s.  A fragment (the rules above) counts when its fp32
 *     depth is less than the opaque picture's depth at that pixel (+inf on background).  Then the word (bits of depth << 32) | id is lowered
 *     into a second word image by integer atomicMin, and (unsigned 64-bit) llrint((2 R_s nz) 2^32) is added to the pixel's thickness word.
 *     Both roads of "render_lane_pixels" exist and give the same words.
 *   3 Smoothing, smooth_iters times, from one fp32 depth image into another (+inf on pixels without liquid, which stay so).  For a liquid pixel
 *     of depth z_p: the offsets dj = -r .. r (outer loop), di = -r .. r (inner loop) in that order; a neighbour q outside the image or without
 *     liquid is skipped; s2 = (double)(di di + dj dj) / (double)((r + 1)(r + 1)), skipped when s2 >= 1; dz = (z_q - z_p) / range, skipped when
 *     dz dz >= 1; w = ((1 - s2)(1 - s2)) ((1 - dz dz)(1 - dz dz)); num = num + w z_q, den = den + w; the result is (float)(num / den) (the
 *     centre has weight 1: den >= 1).  A workgroup owns a 16 x 16 tile and stages it with its halo (at most 32 x 32 floats) in LDS; the order
 *     of the sum is per pixel, so the result does not depend on the tiling.
 *   4 Shade and composite, per pixel with a liquid word.  z = its smoothed depth, d(i, j) the pixel ray of the scene section, P = pos + z d.
 *     Tangent per image direction: among the neighbours at -1 and +1 that are liquid with |z_n - z| < range the one with the smaller
 *     |z_n - z| (a tie: +1) gives t = (pos + z_n d_n) - (pos + z d); with none, the ray at +1 with the pixel's own z.  n = cross(t_y, t_x)
 *     divided by its length (zero or non-finite: -fwd), negated when n.d > 0.  lit = base (ambient + sum c_k max(0, n.l_k)) + specular
 *     sum c_k max(0, n.h_k)^(2^k): base the colour of the word's particle id, l_k the unit vector from P to light k, h_k = l_k - d / |d|
 *     divided by its length.  t = (double)word / 2^32; alpha = alpha_min + ((1 - alpha_min)(absorb t)) / (1 + absorb t); per channel
 *     out = byte(lit alpha + behind (1 - alpha)) with behind = the opaque picture's byte / 255 (the background colour where nothing was
 *     drawn).  The pixel's depth becomes z, its id the liquid particle's, its alpha byte 255.  Pixels without liquid keep the opaque bytes.
 *
 * Contract
 *   - Read-only: no frame, table, sort key or dirty flag changes and a compactly stored F stays compact; a rollout with these calls in it
 *     computes the same frames bit for bit.
 *   - Deterministic: integer atomics only; two draws give the same bytes, and a frame stored in another particle order gives the same bytes.
 *   - Nothing is allocated before fe_surface_set with a non-empty selection; the images follow the size fe_render_setup last set (re-sized at
 *     the next fe_surface_set or fe_surface_frame); fe_destroy frees them.
 *   - Every index read from a pixel word is range-checked before use; no launch has zero workgroups; N = 0 works.
 *   - Errors (non-zero, fe_last_error, the previous state stays, the next picture is the one it would have been): any call before
 *     fe_render_setup; fe_surface_frame before fe_render_set_colors; fe_surface_get before a fe_surface_frame that drew a surface (or after
 *     a later fe_render_setup); a wrong struct size; a parameter outside its range or not finite; 2 R_s N >= 2^31 (a thickness word could
 *     overflow); whatever fe_render_scene_frame refuses.
 * Out of scope: refraction, shadows, anti-aliasing, anisotropic kernels, translucent colliders, gradients through the image, batched engines.
 */
#ifndef FLUIDENGINE_EXT_H
#define FLUIDENGINE_EXT_H

#include "fluidengine.h"

#ifdef __cplusplus
extern "C" {
#endif

/* [N] each, in the caller's particle order; any pointer may be NULL (skipped).  Waits for the engine's stream. */
int fe_param_grad_get(FeEngine* h, double* g_mu, double* g_lam, double* g_rho);
/* the same into DEVICE pointers (memory of the engine's own device) */
int fe_param_grad_get_dev(FeEngine* h, double* g_mu, double* g_lam, double* g_rho);
/* zero the three accumulators and nothing else */
int fe_param_grad_reset(FeEngine* h);

/* observation list: n particle ids in [0, N); duplicates allowed; copied to the device.
   pids == NULL or n == 0 removes the list.  Bad ids: error, list unchanged. */
int fe_obs_set_particles(FeEngine* h, const int* pids, int n);
/* rows i = particle pids[i] of frame f: x [n,3], v [n,3], used [n]; NULL pointers are skipped */
int fe_obs_get(FeEngine* h, int f, fe_real* x, fe_real* v, int* used);       /* host pointers   */
int fe_obs_get_dev(FeEngine* h, int f, fe_real* x, fe_real* v, int* used);   /* device pointers */

#define FE_SUMMARY_MAX_GROUPS 32
/* group[N] by particle id, values in [-1, n_groups); -1 = in no group.
   group == NULL: no groups (only the whole-frame record). */
int fe_summary_set_groups(FeEngine* h, const int* group, int n_groups);

typedef struct FeFrameSummary {
    long long n_used;        /* used particles of the group in frame f */
    long long n_nonfinite;   /* those with a non-finite word in x, v, C or F; excluded from everything below */
    double mass;             /* sum m */
    double com[3];           /* sum m x / mass */
    double momentum[3];      /* sum m v */
    double kinetic;          /* 1/2 sum m |v|^2 */
    double v_max;            /* max over particles and axes of |v_a| */
    double courant;          /* dt * v_max / dx */
    double lo[3], hi[3];     /* bounding box of x */
    double J_min, J_max;     /* range of det F */
} FeFrameSummary;
/* records 0 .. n_groups-1 = the groups; record n_groups = every used particle of the frame (group -1 included).
   Writes min(n_records, n_groups + 1) records.  record_size must equal sizeof(FeFrameSummary). */
int fe_frame_summary(FeEngine* h, int f, FeFrameSummary* out, int n_records, int record_size);

#define FE_TASK_LOSS_MAX_TERMS 8
#define FE_TASK_LOSS_MAX_PAIR_TERMS 2
#define FE_TASK_LOSS_MAX_DENSITY_TERMS 2
#define FE_TASK_LOSS_MAX_NEAREST_TERMS 2
enum { FE_TERM_L1_CONST = 0, FE_TERM_SQ_CONST = 1, FE_TERM_L1_REF = 2, FE_TERM_PAIR_L1 = 3, FE_TERM_DENSITY_SQ = 4, FE_TERM_NEAREST_SQ = 5, FE_TERM_COVER_SQ = 6 };

typedef struct FeLossSel {        /* particles with pid in [pid_lo, pid_hi), of material mat (-1: any), */
    int pid_lo, pid_hi, mat;      /* and, when require_used != 0, with used[f, p] != 0                   */
    int require_used;
} FeLossSel;

typedef struct FeLossTerm {
    int kind;
    int axis_mask;                /* bits 0..2 = x, y, z; at least one */
    FeLossSel a, b;               /* b: FE_TERM_PAIR_L1: b.pid_lo < 0 means all ordered pairs of a with itself; FE_TERM_DENSITY_SQ: b.pid_lo = the field id, the rest 0; FE_TERM_NEAREST_SQ / FE_TERM_COVER_SQ: b.pid_lo = the cloud id, the rest 0 */
    double c[3];                  /* the constant of L1_CONST / SQ_CONST */
    double weight;                /* every constant factor of the term, sign included */
} FeLossTerm;

/* step_loss[max_loss_steps] and term_loss[FE_TASK_LOSS_MAX_TERMS][max_loss_steps], fp64 on the device, zeroed */
int fe_task_loss_alloc(FeEngine* h, int max_loss_steps);
/* the program: n_terms terms of term_size == sizeof(FeLossTerm) bytes each; n_terms == 0 removes it */
int fe_task_loss_set_terms(FeEngine* h, const FeLossTerm* terms, int n_terms, int term_size);
/* ref[pid] = x[f, pid] for every pid, copied on the device */
int fe_task_loss_set_ref(FeEngine* h, int f);
/* zero step_loss and term_loss */
int fe_task_loss_clear(FeEngine* h);
/* step_loss[s] += sum_t value_t(f);  term_loss[t][s] += value_t(f) */
int fe_task_loss_step(FeEngine* h, int s, int f);
/* x.grad[f, p] += (float)(scale * sum_t d value_t / d x_p) */
int fe_task_loss_step_grad(FeEngine* h, int s, int f, double scale);
/* step_loss[s0 .. s0 + n) and term_loss as [n_terms][n] (may be NULL) to the host; waits for the stream */
int fe_task_loss_get(FeEngine* h, int s0, int n, double* step_loss, double* term_loss);

#define FE_DENSITY_MAX_FIELDS 2
#define FE_DENSITY_MAX_CELLS (1 << 21)
#define FE_DENSITY_LDS_CELLS 8192
typedef struct FeDensitySpec {
    double origin[3];             /* the corner of cell (0, 0, 0) */
    double cell[3];               /* cell size per axis, finite and positive */
    int n[3];                     /* cells per axis, >= 1; 1 = projected along that axis */
    int pad;
} FeDensitySpec;
/* spec_size must equal sizeof(FeDensitySpec); spec == NULL removes the field.  Setting a field drops its target. */
int fe_density_set_field(FeEngine* h, int field, const FeDensitySpec* spec, int spec_size);
/* target[n_cells] by linear cell index, copied to the device; n_cells must be the field's cell count */
int fe_density_set_target(FeEngine* h, int field, const double* target, long long n_cells);
/* out[n_cells] = D of frame f from the particles selected by sel (NULL: every used particle); waits for the stream */
int fe_density_get(FeEngine* h, int f, int field, const FeLossSel* sel, double* out, long long n_cells);

#define FE_CLOUD_MAX 4
#define FE_CLOUD_MAX_POINTS (1 << 20)
#define FE_CLOUD_COORD_MAX 2.0
/* cloud `cloud` = n points, xyz[n][3], copied to the device; n == 0 or xyz == NULL removes it */
int fe_cloud_set(FeEngine* h, int cloud, const float* xyz, int n);
/* frame f against the cloud, on the axes of axis_mask, for the particles selected by sel (NULL: every used particle):
   nn_of_particle[N] by pid = the index of the nearest cloud point (-1: the particle is not a query), d2_of_particle[N] its d2 (0 there);
   nn_of_point[n] = the pid of the nearest selected particle (-1: there is none), d2_of_point[n] its d2 (0 there).
   Any pointer may be NULL.  Waits for the stream. */
int fe_cloud_query(FeEngine* h, int f, int cloud, const FeLossSel* sel, int axis_mask,
                   int* nn_of_particle, double* d2_of_particle, int* nn_of_point, double* d2_of_point);

#define FE_SMOKE_MAX_LISTS 4
#define FE_SMOKE_MAX_LIST_CELLS (1 << 16)
enum { FE_SMOKE_L1 = 0, FE_SMOKE_SQ = 1 };

/* list `list` = n cells, cells[n][3] = (i, j, k) in [0, res); duplicates allowed; copied to the device.
   cells == NULL or n == 0 removes the list.  A bad cell or n: error, list unchanged. */
int fe_smoke_cells_set(FeEngine* h, int list, const int* cells, int n);
/* rows i = cell i of the list in smoke frame s: v [n,3], q [n,q_dim]; NULL pointers are skipped */
int fe_smoke_cells_get(FeEngine* h, int list, int s, fe_real* v, fe_real* q);       /* host pointers; waits */
int fe_smoke_cells_get_dev(FeEngine* h, int list, int s, fe_real* v, fe_real* q);   /* device pointers     */
/* the adjoint of those reads: row i of gv [n,3] / gq [n,q_dim] is added to the v / q adjoint of cell i of the list in smoke frame s;
   NULL pointers are skipped, with both NULL nothing is launched */
int fe_smoke_cells_add_grad(FeEngine* h, int list, int s, const fe_real* gv, const fe_real* gq);       /* host pointers; waits */
int fe_smoke_cells_add_grad_dev(FeEngine* h, int list, int s, const fe_real* gv, const fe_real* gq);   /* device pointers     */

/* step_loss[max_loss_steps], fp64 on the device, zeroed */
int fe_smoke_loss_alloc(FeEngine* h, int max_loss_steps);
/* the detectors: the cells of `list` (no duplicates), component comp of q, kind FE_SMOKE_L1 or FE_SMOKE_SQ,
   target[n] and weight[n] (NULL = 1) copied to the device */
int fe_smoke_loss_set(FeEngine* h, int list, int comp, int kind, const double* target, const double* weight);
/* zero step_loss */
int fe_smoke_loss_clear(FeEngine* h);
/* step_loss[s_loss] += sum_i w_i |q[s, cell_i, comp] - t_i|   (FE_SMOKE_SQ: squared) */
int fe_smoke_loss_step(FeEngine* h, int s_loss, int s);
/* gq[s, cell_i, comp] += (float)(scale * w_i * sign(d_i))      (FE_SMOKE_SQ: 2 d_i) */
int fe_smoke_loss_step_grad(FeEngine* h, int s_loss, int s, double scale);
/* step_loss[s0 .. s0 + n) to the host; waits for the stream */
int fe_smoke_loss_get(FeEngine* h, int s0, int n, double* step_loss);

typedef struct FeSmokeSummary {
    long long n_cells;       /* cells of the slab lower_y < j < higher_y */
    long long n_nonfinite;   /* those with a non-finite word in v or q; excluded from everything below */
    double v_max;            /* max over cells and axes of |v_a| */
    double courant;          /* dt * v_max */
    double kinetic;          /* 1/2 sum |v|^2 */
    double q_sum[3], q_min[3], q_max[3];   /* per component of q; entries beyond q_dim are zero */
} FeSmokeSummary;
/* record_size must equal sizeof(FeSmokeSummary).  Waits for the stream. */
int fe_smoke_summary(FeEngine* h, int s, FeSmokeSummary* out, int record_size);

#define FE_RENDER_MAX_LIGHTS 4
#define FE_RENDER_MAX_SETS 2
#define FE_RENDER_MAX_POINTS (1 << 20)
#define FE_RENDER_MAX_SIZE 4096
/* boxes of more pixels than this are drawn by the whole wave.  Chosen as a guess; profiles/render_cost.txt (scripts/render_cost.py) found the
   two roads within 7 % of each other, neither ahead, on the benchmark block at 960 x 960, where boxes are about 5 x 5, so it has not been moved. */
#define FE_RENDER_LANE_PIXELS 25
typedef struct FeRenderCamera {
    double pos[3];
    double right[3], up[3], fwd[3];   /* orthonormal */
    double focal;                     /* pixels: 0.5 height / tan(fov_y / 2) */
    double near;                      /* spheres with zc <= near + R are dropped */
    double max_radius_px;             /* projected radii are clamped to this (32: a particle at the lens cannot cover the image) */
    int width, height;                /* [1, FE_RENDER_MAX_SIZE] */
} FeRenderCamera;
typedef struct FeRenderLights {
    double ambient[3];
    double background[3];
    double pos[FE_RENDER_MAX_LIGHTS][3];
    double color[FE_RENDER_MAX_LIGHTS][3];
    int n_lights, pad;
} FeRenderLights;
/* camera_size == sizeof(FeRenderCamera), lights_size == sizeof(FeRenderLights); allocates the image buffers */
int fe_render_setup(FeEngine* h, const FeRenderCamera* camera, int camera_size, const FeRenderLights* lights, int lights_size);
/* rgba[N][4] by particle id, copied to the device; radius: the particles' world radius */
int fe_render_set_colors(FeEngine* h, const unsigned char* rgba, double radius);
/* point set `set`: xyz[n][3], one colour rgba[4] and a world radius; xyz == NULL or n == 0 removes the set */
int fe_render_set_points(FeEngine* h, int set, const float* xyz, int n, const unsigned char* rgba, double radius);
/* enqueue the picture of frame f; does not wait */
int fe_render_frame(FeEngine* h, int f);
/* the last picture: rgba [H][W][4], depth [H][W], id [H][W]; NULL pointers are skipped */
int fe_render_get(FeEngine* h, unsigned char* rgba, float* depth, int* id);       /* host pointers; waits */
int fe_render_get_dev(FeEngine* h, unsigned char* rgba, float* depth, int* id);   /* device pointers     */

#define FE_RENDER_MAX_VOLUMES 16
enum { FE_RENDER_VOL_NONE = 0, FE_RENDER_VOL_STATIC = 1, FE_RENDER_VOL_EFFECTOR = 2, FE_RENDER_VOL_OWN = 3 };
typedef struct FeRenderScene {
    double march_step;                /* voxels per sample of the march, in (0, 1]; 0.5 */
    double smoke_radius;              /* world radius of a cell's sphere (the reference: 1/128; the host passes 1 / n_grid) */
    double cold[3], hot[3];           /* a cell's base colour is cold (1 - q) + hot q */
    int bisect_iters;                 /* [0, 32]; 10 */
    int draw_smoke;                   /* != 0: one sphere per cell of the slab */
    int lo, hi;                       /* the visible slab lo < j < hi, inside [-1, res] */
} FeRenderScene;
/* slot [0, FE_RENDER_MAX_VOLUMES): source FE_RENDER_VOL_STATIC (index = the static fe_add_static returned), _EFFECTOR (index = the effector;
   it must have a mesh), _OWN (desc and voxels as fe_add_static takes them, copied) or _NONE (clears the slot); rgba[4] */
extern int fe_render_set_volume(FeEngine* h, int slot, int source, int index, const FeSdfDesc* desc, const fe_real* voxels, const unsigned char* rgba);
/* scene_size == sizeof(FeRenderScene); scene == NULL: no scene (march_step and bisect_iters return to their defaults) */
extern int fe_render_set_scene(FeEngine* h, const FeRenderScene* scene, int scene_size);
/* enqueue the picture of frame f with the volumes and smoke frame s in it; does not wait */
extern int fe_render_scene_frame(FeEngine* h, int f, int s);

typedef struct FeContactRecord {
    double impulse[3];       /* sum of m (v_after - v_before): what the collider gave to the material in this substep */
    double ang_impulse[3];   /* sum of r x m (v_after - v_before) about the world origin */
    double ref[3];           /* effector: its position words at frame f; static: 0 */
    long long n_particles;   /* particle-level contacts counted */
    long long n_nodes;       /* node-level contacts counted */
    int valid;               /* 1: frame f has its grid in the store; 0: it has not, everything above is zero */
    int kind;                /* 0 effector, 1 static */
} FeContactRecord;
/* records per substep: the effectors 0 .. n_eff-1 (one without a mesh gives zeros, valid as the frame's), then the statics.
   out[(f - f0) * n_records + c]; writes min(n_records, n_eff + n_static) per substep; waits for the stream. */
extern int fe_contact_count(FeEngine* h);      /* n_eff + n_static */
/* record_size must equal sizeof(FeContactRecord) */
extern int fe_contact_wrench(FeEngine* h, int f0, int n, FeContactRecord* out, int n_records, int record_size);

/*
 * Closed-loop policies: observation and tool-state adjoints (fluidlab_amd/csrc/fe_policy_io.h)
 * ---------------------------------------------------------------------------------------------
 * A policy a_i = pi(o_i) is trained through the simulator by adding dL/do_i to the adjoint of the frame o_i was read from before the
 * reverse sweep goes on.  These entries carry that cotangent, and the three per-step crossings of such a loop, without dense [N, 3] arrays
 * and -- in their _dev forms -- without the host.
 *
 *   fe_obs_add_grad(h, f, gx, gv)          gx, gv [n][3] (either may be NULL), n the length of the list given to fe_obs_set_particles: row i
 *                                          is added to the x / v adjoint of particle pids[i] of frame f.  Duplicates in the list are legal:
 *                                          a particle's rows are summed in list order in fp32, starting from 0, and the sum is added to the
 *                                          slot once, by the one thread that owns the particle (the rows are grouped once per list).  No
 *                                          floating-point atomics: the result does not depend on launch geometry or timing.  The slot is
 *                                          found through the adjoint slot's own particle order (a cleared slot takes the frame's).  Only the
 *                                          x and v words change; a compactly stored F adjoint stays compact.
 *   fe_eff_add_state_grad(h, e, f, g7)     gpos[f] += g7[0..3), gquat[f] += g7[3..7) of effector e;  fe_eff_get_state_grad reads the seven.
 *   fe_eff_get_state_dev(h, e, f, s7)      pos[f], quat[f] into seven device floats.
 *   fe_eff_set_action_dev(...)             fe_eff_set_action with the action_dim action words read from device memory: the same kernel
 *                                          body, the same abuf, v, w (and AirCon s, r) for the same numbers.
 *   fe_eff_get_action_grad_dev(h,e,s,n,g)  gabuf[s .. s + n) -- n * action_dim words -- to a device pointer (the position part, gabuf_p,
 *                                          is not included).
 * The host variants stage through the engine; every call returns after the engine's stream has drained.  Errors (non-zero, fe_last_error,
 * nothing changed): no observation list, f or e out of range, a frame whose adjoint a fused fe_step_grad passed on in registers (as
 * fe_add_grad), a NULL pointer where one is needed.  Nothing is allocated before the first call; fe_destroy frees everything.
 * Out of scope: batched forms, adjoints of `used` and of an Injector's act_id.  (The smoke field's observation has its adjoint entry with
 * the smoke-field reads above, fe_smoke_cells_add_grad; the loop on Circulation-v0 goes through fe_smoke_obs_* below.)
 */
extern int fe_obs_add_grad(FeEngine* h, int f, const fe_real* gx, const fe_real* gv);          /* host pointers   */
extern int fe_obs_add_grad_dev(FeEngine* h, int f, const fe_real* gx, const fe_real* gv);      /* device pointers */
extern int fe_eff_add_state_grad(FeEngine* h, int e, int f, const fe_real* g7);                /* host pointer    */
extern int fe_eff_add_state_grad_dev(FeEngine* h, int e, int f, const fe_real* g7);            /* device pointer  */
extern int fe_eff_get_state_grad(FeEngine* h, int e, int f, fe_real* g7);                      /* host pointer    */
extern int fe_eff_get_state_dev(FeEngine* h, int e, int f, fe_real* s7);                       /* device pointer  */
extern int fe_eff_set_action_dev(FeEngine* h, int e, int s, int s_global, int n_substeps, const fe_real* action);   /* device pointer */
extern int fe_eff_get_action_grad_dev(FeEngine* h, int e, int s, int n, fe_real* grad);        /* device pointer  */

/*
 * Closed-loop policies on Circulation-v0: the observation vector and its cotangent, one device call each
 * ---------------------------------------------------------------------------------------------------------
 * The vector CirculationEnv observes is the AirCon's state at local frame f (pos 3, quat 4, strength s, radius r: FE_SMOKE_OBS_STATE
 * words), then the v rows [n][3] of cell list `list` in smoke frame s, then its q rows [n][q_dim]: n_out = 9 + n (3 + q_dim) words.
 *
 *   fe_smoke_obs_get(h, list, s, eff, f, out, n_out)       one launch (k_smoke_obs_pack) writes the whole vector; the words are the
 *                                                          frame's and the effector's fp32 words.  The host form waits; _dev enqueues
 *                                                          like fe_smoke_cells_get_dev.
 *   fe_smoke_obs_add_grad(h, list, s, eff, f, g, n_g)      the adjoint, one launch (k_smoke_obs_scatter_grad): the v / q rows of g are
 *                                                          added to gv[s] / gq[s] at the list's cells exactly as
 *                                                          fe_smoke_cells_add_grad does it (one thread per distinct cell, rows summed in
 *                                                          list order in fp32 from 0, added once); g[0..7) is added to gpos[f], gquat[f]
 *                                                          as fe_eff_add_state_grad does it; g[7], g[8] to the AirCon's gsa[f], gra[f],
 *                                                          from where the adjoint of the effector's move carries them into gabuf.  The
 *                                                          same bits as the composition of those calls.  No floating-point atomics.
 *   fe_eff_add_sr_grad(h, e, f, gs, gr)                    gsa[f] += gs, gra[f] += gr of AirCon e;  fe_eff_get_sr_grad reads the two.
 * Errors (non-zero, fe_last_error, no adjoint word changed): no smoke field, a list that is not set, s or f out of range, an effector
 * index out of range or one that is not an AirCon, n_out / n_g that is not the vector's length, a NULL pointer.
 */
#define FE_SMOKE_OBS_STATE 9
extern int fe_smoke_obs_get(FeEngine* h, int list, int s, int eff, int f, fe_real* out, int n_out);               /* host pointer; waits */
extern int fe_smoke_obs_get_dev(FeEngine* h, int list, int s, int eff, int f, fe_real* out, int n_out);           /* device pointer      */
extern int fe_smoke_obs_add_grad(FeEngine* h, int list, int s, int eff, int f, const fe_real* g, int n_g);        /* host pointer; waits */
extern int fe_smoke_obs_add_grad_dev(FeEngine* h, int list, int s, int eff, int f, const fe_real* g, int n_g);    /* device pointer      */
extern int fe_eff_add_sr_grad(FeEngine* h, int e, int f, fe_real gs, fe_real gr);
extern int fe_eff_get_sr_grad(FeEngine* h, int e, int f, fe_real* gs, fe_real* gr);                               /* host pointers       */

/*
 * Field observations: density and momentum grids of a frame, with adjoints (fluidlab_amd/csrc/fe_field_obs.h)
 * -------------------------------------------------------------------------------------------------------------
 * The observation of fe_obs_get is a list of particle ids.  An observation field is the Eulerian counterpart: a FeDensitySpec box, a
 * FeLossSel selection and a channel count C (1 or 4).  It is permutation-invariant and has a fixed size.  FE_FIELD_OBS_MAX fields, kept
 * apart from the loss fields of fe_density_set_field.  The stencil, the dropped cells and the projected axes are the density fields'.
 *   channel 0       D_c   = sum_p w_pc            (the same words as fe_density_get of the same box and selection)
 *   channels 1..3   P_c,a = sum_p w_pc v_p,a      (momentum with a particle's mass taken as 1; a policy that wants velocity divides)
 *
 *   fe_field_obs_set(h, k, spec, spec_size, sel, channels)   defines field k (sel == NULL: every used particle); spec == NULL removes it
 *   fe_field_obs_get(h, f, k, out, n_values)                 the field of frame f, [C][n0][n1][n2] in fp64, to the host; waits
 *   fe_field_obs_get_dev(h, f, k, out)                       the same as fe_real values (converted through fp64) through a device pointer;
 *                                                            returns after the engine's stream has drained, as fe_obs_get_dev does
 *   fe_field_obs_add_grad(h, f, k, G)                        G [C][n0][n1][n2] in fe_real: a selected particle that passes the guards gets
 *                                                              gx_a += sum_c (G_0[c] + sum_b G_{1+b}[c] v_b) d w_pc / d x_a
 *                                                              gv_b += sum_c G_{1+b}[c] w_pc                                  (C == 4)
 *                                                            summed in fp64 over the in-field stencil cells in the fixed order i, j, k, rounded
 *                                                            to fp32 once and added to the adjoint slot once, by the one thread that owns
 *                                                            the particle.  x and v are read from frame f in the frame's order; the slot is
 *                                                            found through the adjoint slot's own particle order (a cleared slot takes the
 *                                                            frame's).  Only the x and v words change; a compact F adjoint stays compact.
 *                                                            _dev: G through a device pointer.  Both return after the stream has drained.
 * Contract
 *   - Fixed point: a density deposit is llrint(w 2^40) into an unsigned 64-bit word; a momentum deposit is llrint(w v_a 2^28) as a signed
 *     64-bit integer added in two's complement, decoded as (double)(long long)word / 2^28.  Every deposit is within 2^-29 of exact, a cell
 *     with k_c deposits within k_c 2^-29.  A field is the same bits however it was accumulated: in per-workgroup LDS copies of all channels
 *     (when C * 8 * cells fits the device's LDS per workgroup) or straight with 64-bit integer global atomics.  Option "field_obs_lds": -1 the
 *     engine chooses (the LDS road whenever the field fits: measured faster or equal, profiles/field_obs_cost.txt), 0 never the LDS road,
 *     1 whenever the field fits.  No floating-point atomics anywhere.
 *   - A particle deposits nothing in any channel, and gets no gradient, when the density guard drops it (a non-finite position word,
 *     |u| > 2^30), when a velocity word is not finite, or when |v_a| > 2^10 on any axis -- whatever C is.  With N <= 2^23 a momentum word
 *     stays below 2^61.
 *   - The calls only read the frame: no table, key, flag or frame word changes.  Nothing is allocated before fe_field_obs_set.
 *   - Errors (non-zero, fe_last_error, every field and every adjoint as it was): a field id out of range, a wrong spec_size, n[a] < 1, more
 *     than FE_DENSITY_MAX_CELLS cells, a cell size or origin that is not finite (cell: and positive), channels not 1 or 4, a selection
 *     outside [0, N], N > 2^23, a field that is not set, an n_values that is not C * cells, a NULL pointer, a frame whose adjoint a fused
 *     fe_step_grad passed on in registers (as fe_add_grad).
 * Out of scope: batched forms, gradients with respect to the spec.
 */
#define FE_FIELD_OBS_MAX 4
extern int fe_field_obs_set(FeEngine* h, int k, const FeDensitySpec* spec, int spec_size, const FeLossSel* sel, int channels);
extern int fe_field_obs_get(FeEngine* h, int f, int k, double* out, long long n_values);       /* host pointer; waits */
extern int fe_field_obs_get_dev(FeEngine* h, int f, int k, fe_real* out);                      /* device pointer      */
extern int fe_field_obs_add_grad(FeEngine* h, int f, int k, const fe_real* G);                 /* host pointer; waits */
extern int fe_field_obs_add_grad_dev(FeEngine* h, int f, int k, const fe_real* G);             /* device pointer      */

/* Liquids as a smoothed, translucent surface ("Liquids in that picture" above; fluidlab_amd/csrc/fe_surface.h) */
typedef struct FeSurfaceParams {
    double radius_scale;              /* >= 1: liquid spheres are drawn with radius_scale * radius */
    double range;                     /* > 0, depth units: neighbours further apart in depth are not blended */
    double absorb;                    /* >= 0, per unit length of liquid along the ray */
    double alpha_min;                 /* [0, 1]: the opacity of a vanishing thickness */
    double specular;                  /* [0, 1]: the weight of the highlight */
    int smooth_iters;                 /* [0, 8] passes */
    int smooth_radius_px;             /* [1, 8]: the window is (2 r + 1)^2 pixels */
    int shininess_log2;               /* [0, 10]: the highlight is max(0, n.h)^(2^shininess_log2) */
    int pad;
} FeSurfaceParams;
/* sel[N] by particle id, != 0: drawn as liquid; params_size == sizeof(FeSurfaceParams); sel == NULL or all zero: the surface is off */
extern int fe_surface_set(FeEngine* h, const unsigned char* sel, const FeSurfaceParams* params, int params_size);
/* enqueue the picture fe_render_scene_frame(f, s) would give, with the surface; does not wait */
extern int fe_surface_frame(FeEngine* h, int f, int s);
/* the liquid layer of the last fe_surface_frame: z_raw [H][W], z_smooth [H][W] (+inf without liquid), thickness [H][W]; NULL pointers are skipped */
extern int fe_surface_get(FeEngine* h, float* z_raw, float* z_smooth, double* thickness);       /* host pointers; waits */
extern int fe_surface_get_dev(FeEngine* h, float* z_raw, float* z_smooth, double* thickness);   /* device pointers     */

#ifdef __cplusplus
}
#endif
#endif /* FLUIDENGINE_EXT_H */
