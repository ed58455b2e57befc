/*
 * co_env.h -- C ABI of the MI355X (gfx950) batched CO-environment engine.
 *
 * Drop-in boundary for the rl4co-slap hot path: the per-step env functions of
 * TSP / CVRP / SLAP, the episode-end rewards + validity checks, the fused
 * decode step and utils.ops.gather_by_index.  Each entry point replaces the
 * ATen op sequence the reference issues at the cited file:line of
 * j4n1k/rl4co-slap (reference @ 2025-02-02).
 *
 * Conventions (all entry points):
 *  - plain device pointers + sizes; no torch / HIP types in the signatures;
 *    `stream` is a hipStream_t passed as void* (NULL = default stream);
 *  - every call is stream-ordered and asynchronous: no allocation, no host
 *    synchronisation, graph-capturable; the library never owns user memory;
 *  - the caller allocates every output; outputs may alias their matching input
 *    only where a parameter comment says so ("in-place allowed");
 *  - return 0 on success, CO_E_* (< 0) for invalid arguments, or the positive
 *    hipError_t of a failed launch.  Nothing throws across the ABI;
 *  - data-dependent failures (invalid tour, capacity overflow, infeasible or
 *    out-of-range index) are OR-ed into a caller-provided device word
 *    `status` (bits CO_ST_*); the host maps them to the reference's
 *    AssertionError / IndexError messages;
 *  - dtypes are the reference TensorDict dtypes: bool/uint8 masks as bytes,
 *    int64 indices, float32 coordinates/demands/rewards, int32 assignment.
 */
#ifndef CO_ENV_H
#define CO_ENV_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CO_OK 0
#define CO_E_INVAL (-1)     /* bad size / null pointer */
#define CO_E_ALIGN (-2)     /* pointer misaligned for its dtype */
#define CO_E_MODE (-3)      /* unknown mode */

/* status bits (device int32, OR-ed atomically) */
#define CO_ST_INVALID_TOUR 1      /* "Invalid tour"              tsp/env.py:173, cvrp/env.py:175 */
#define CO_ST_OVER_CAPACITY 2     /* "Used more than capacity"   cvrp/env.py:188-190 */
#define CO_ST_INFEASIBLE 4        /* "infeasible action selected" decoding.py:376-379 */
#define CO_ST_INDEX_RANGE 8       /* index out of range (torch raises IndexError/RuntimeError) */
#define CO_ST_TRUNCATED 16        /* an episode hit max_steps before done (rollout max_steps) */
#define CO_ST_LOGP_NEG_INF 32     /* "Logprobs should not be -inf, ..."  decoding.py:57-58 */

/* Library identification: returns the gfx target string compiled in. */
const char* co_build_info(void);

/* ------------------------------------------------------------------ TSP */

/* TSPEnv._reset (rl4co/envs/routing/tsp/env.py:95-120):
 * action_mask[B,N] = 1, first_node[B] = current_node[B] = 0, i[B,1] = 0,
 * reward[B,1] = 0.  first_node and current_node may be the same buffer
 * (the reference aliases them). */
int co_tsp_reset(int64_t batch, int64_t num_loc, uint8_t* action_mask, int64_t* first_node,
                 int64_t* current_node, int64_t* i, float* reward, void* stream);

/* TSPEnv._step (tsp/env.py:67-93):
 *   first_out = (first_mode says the batch has an i == 0) ? action : first_in
 *   mask_out  = mask_in with mask_out[b, action[b]] = 0       (in-place allowed)
 *   done[b]   = sum(mask_out[b]) == 0 ; reward[b] = 0 (bool)
 *   i_out     = i_in + 1 (in-place allowed); current_out = action (may be NULL)
 * first_mode: 0 = keep first_in, 1 = take action, 2 = read *first_flag (device
 * int32, nonzero = take action; produced by co_any_eq_i64).  This is the
 * batch-wide `td["i"].all() == 0` test of tsp/env.py:70. */
int co_tsp_step(int64_t batch, int64_t num_loc, const int64_t* action, const uint8_t* mask_in,
                uint8_t* mask_out, const int64_t* i_in, int64_t* i_out, const int64_t* first_in,
                int64_t* first_out, int64_t* current_out, uint8_t* done, uint8_t* reward,
                int first_mode, const int32_t* first_flag, int32_t* status, void* stream);

/* K consecutive TSPEnv._step calls (tsp/env.py:67-93) in one launch (round 6): exactly the
 * K co_tsp_step launches t = 0..K-1 with action row t at action + t*act_stride and the
 * state ping-ponging between buffers A and B (step t reads A and writes B for even t, the
 * reverse for odd t; current_out / done / reward written by every step), so every step's
 * state is stored as its own launch would store it and the final contents are
 * bit-identical.  first_mode (step 0 only): 0 = keep first_a, 1 = take action (the
 * episode's first step).  Rows the lane-group kernel does not take (N % 4 != 0, tiny N)
 * run as the K single-step launches.  Replaces K env.step() calls of a loop whose actions
 * are known in advance (teacher forcing, the stepwise engine). */
int co_tsp_steps(int64_t batch, int64_t num_loc, int64_t steps, const int64_t* action,
                 int64_t act_stride, uint8_t* mask_a, int64_t* i_a, int64_t* first_a,
                 uint8_t* mask_b, int64_t* i_b, int64_t* first_b, int64_t* current_out,
                 uint8_t* done, uint8_t* reward, int first_mode, int32_t* status, void* stream);

/* TSPEnv.get_reward (envs/common/base.py:182-188 + tsp/env.py:157-173):
 * reward[b] = -closed tour length of locs[b % locs_batch, actions[b, 0..T-1]]
 * (locs_batch = batch normally; = instances for the POMO [S, B] multistart layout,
 * which then reads each instance's coordinates without batchify's copy, ops.py:16).
 * actions element (b, t) lives at actions[b*act_stride_b + t*act_stride_t].
 * check != 0: a row that is not a permutation of 0..T-1 sets CO_ST_INVALID_TOUR
 * (the reference's sort(1) == arange(T) test). */
int co_tsp_reward(int64_t batch, int64_t num_loc, int64_t steps, const float* locs,
                  int64_t locs_batch, const int64_t* actions, int64_t act_stride_b, int64_t act_stride_t, int check,
                  float* reward, int32_t* status, void* stream);

/* TSPEnv.local_search (tsp/env.py:192-197 -> tsp/local_search.py:14-74): best-improvement
 * 2-opt on every row, the whole search of a row in one launch.  Per sweep every move
 * (i, j), 1 <= i < j <= n-1 (n = num_loc tour positions), is scored in f32, left to right,
 *   change = ((D[t[i-1],t[j]] + D[t[i],t[(j+1)%n]]) - D[t[i-1],t[i]]) - D[t[j],t[(j+1)%n]]
 * the smallest change (equal values: the lexicographically first (i, j)) is taken, and
 * when it is < -1e-6 (compared in double) t[i..j] is reversed; the search ends with the
 * first sweep that does not improve or after max_iterations sweeps.
 * D (row = first operand) is distances[b % locs_batch] (f32 [locs_batch, n, n]) or, with
 * locs (f32 [locs_batch, n, 2]), the f32 Euclidean sqrt(dx*dx + dy*dy) co_distance_matrix
 * writes; exactly one of locs / distances is non-NULL.  actions element (b, k) lives at
 * actions[b*act_stride_b + k*act_stride_t] (row-major or step-major, as co_tsp_reward).
 * actions_out[batch, n] (row-major; must not alias actions) receives the improved tours,
 * sweeps_out[batch] (nullable) the sweeps executed (the reference's `iterations`).
 * max_iterations <= 0 copies the input (0 sweeps), n < 3 has no move (the input after 1
 * sweep); max_iterations above 2^31 - 1 counts as 2^31 - 1.  A row that is not a
 * permutation of 0..n-1 sets CO_ST_INVALID_TOUR and is copied unchanged with 0 sweeps (the
 * reference has no such check: its uint16 cast and skip test leave such rows
 * unspecified).  num_loc <= CO_TWO_OPT_MAX_N, else
 * CO_E_INVAL.  One wavefront per row, tour state in LDS; a distances matrix of
 * n <= CO_TWO_OPT_STAGE_N is staged in LDS, larger ones are read through L2. */
#define CO_TWO_OPT_MAX_N 1024
#define CO_TWO_OPT_STAGE_N 126
int co_tsp_two_opt(int64_t batch, int64_t num_loc, const float* locs, const float* distances,
                   int64_t locs_batch, const int64_t* actions, int64_t act_stride_b,
                   int64_t act_stride_t, int64_t max_iterations, int64_t* actions_out,
                   int32_t* sweeps_out, int32_t* status, void* stream);

/* 2-opt + Or-opt descent on every row, the whole search of a row in one launch (the
 * reference has 2-opt only; Or-opt is the classical "move a short chain elsewhere"
 * companion).  The arguments are co_tsp_two_opt's plus `operators`, a mask of
 * CO_TSP_LS_TWO_OPT | CO_TSP_LS_OR_OPT (0 or an unknown bit: CO_E_INVAL), and moves_out
 * (nullable, int32 [batch, 2]): the applied 2-opt and the applied Or-opt moves per row.
 * num_loc <= CO_TWO_OPT_MAX_N, exactly one of locs / distances, locs_batch, the action
 * strides, actions_out not aliasing actions, the CO_E_* returns, the empty batch (a no-op)
 * and the LDS staging of a matrix of n <= CO_TWO_OPT_STAGE_N are as co_tsp_two_opt has
 * them, and D is the same: the given matrix (row = first operand) or the f32
 * sqrt(dx*dx + dy*dy) of the coordinates.
 *
 * Or-opt neighbourhood.  The tour t has n cyclic positions.  A move is (L, i, k, rev):
 * the segment t[i..i+L-1] of length L in {1, 2, 3}, 1 <= i and i+L-1 <= n-1 (position 0
 * never moves, as in 2-opt), is taken out and reinserted -- reversed if rev = 1; L = 1 has
 * rev = 0 only -- directly after node c = t[k], into the edge (t[k], t[(k+1)%n]) with
 * 0 <= k <= n-1 and k not in [i-1, i+L-1].  With a = t[i-1], s1 = t[i], s2 = t[i+L-1],
 * b = t[(i+L)%n], d = t[(k+1)%n] and (x, y) = (s1, s2) for rev = 0, (s2, s1) for rev = 1,
 * the move is scored in f32, left to right, every operation rounded on its own (no FMA):
 *   change = ((((D[a,b] + D[c,x]) + D[y,d]) - D[a,s1]) - D[s2,b]) - D[c,d]
 * (as with 2-opt on an asymmetric matrix, the interior edges of a reversed segment are
 * ignored: the formula is the definition).  An L without an admissible (i, k) -- n - L - 1
 * < 1, or no i -- is skipped.
 *
 * Descent.  A sweep: if TWO_OPT is enabled, the 2-opt neighbourhood is scored exactly as
 * in co_tsp_two_opt, the smallest change (equal values: the lexicographically first
 * (i, j)) is taken and applied if (double)change < -1e-6.  If this sweep applied no 2-opt
 * move and OR_OPT is enabled, the Or-opt neighbourhood is scored; the smallest change --
 * on equal values the first in the order L ascending, then i, then k, then rev 0 before 1:
 * a strict `<` against a running minimum that starts at 0 -- is applied if (double)change
 * < -1e-6.  The search ends with the first sweep that applies nothing or after
 * max_iterations sweeps; sweeps_out counts sweeps (one that scans both neighbourhoods
 * counts once).  So with operators == CO_TSP_LS_TWO_OPT tours and sweeps are
 * co_tsp_two_opt's, and with both bits the run starts with the 2-opt-only run.
 * A row that is not a permutation (copied, 0 sweeps, CO_ST_INVALID_TOUR),
 * max_iterations <= 0, n < 3 and the clamping of max_iterations are as in co_tsp_two_opt;
 * such rows report 0 moves. */
#define CO_TSP_LS_TWO_OPT 1
#define CO_TSP_LS_OR_OPT 2
int co_tsp_local_search(int64_t batch, int64_t num_loc, const float* locs,
                        const float* distances, int64_t locs_batch, const int64_t* actions,
                        int64_t act_stride_b, int64_t act_stride_t, int64_t max_iterations,
                        int operators, int64_t* actions_out, int32_t* sweeps_out,
                        int32_t* moves_out, int32_t* status, void* stream);

/* ------------------------------------------- TSP k-opt improvement MDP
 * TSPkoptEnv (tsp/env.py:204-549) on ImprovementEnvBase (envs/common/base.py:336-403).
 * A solution is a linked list rec (int64 [B, N]): rec[i] = j means edge i -> j; pred is the
 * inverse of rec.  A valid rec is one N-cycle.  num_loc <= CO_KOPT_MAX_N and, where an
 * action is given, 2 <= k_max <= CO_KOPT_MAX_K, else CO_E_INVAL; an empty batch is a no-op.
 * D(a, c) is the f32 sqrt(dx*dx + dy*dy) of the coordinates (no FMA), locs f32
 * [locs_batch, N, 2] with row b reading instance b % locs_batch, as co_tsp_reward.
 * The cost of a row is sum over nodes i (not tour positions) of D(i, rec[i]), added in f64
 * and rounded once to f32 as co_tsp_reward adds: a function of the (locs row, rec row) pair
 * alone, so an unchanged rec has a bit-identical cost in every entry below.
 * One wavefront per row, rec / positions / order in LDS; positions come from rec by
 * pointer jumping (log2 N rounds). */
#define CO_KOPT_MAX_N 1024
#define CO_KOPT_MAX_K 16

/* ImprovementEnvBase._get_linked_list_solution (base.py:386-393): rec[b, t[k]] =
 * t[(k+1) % N] for the tour row t, element (b, k) at tour[b*stride_b + k*stride_t] (as
 * co_tsp_reward's actions).  A row that is not a permutation of 0..N-1 sets
 * CO_ST_INVALID_TOUR and is not written.  rec must not alias tour. */
int co_tsp_linked_list(int64_t batch, int64_t num_loc, const int64_t* tour, int64_t stride_b,
                       int64_t stride_t, int64_t* rec, int32_t* status, void* stream);

/* ImprovementEnvBase._get_real_solution (base.py:371-384): solution[b] = the visiting
 * order [0, rec[0], rec[rec[0]], ...] (int64 [B, N]).  A rec that is not one N-cycle sets
 * CO_ST_INVALID_TOUR; the row is then not written. */
int co_tsp_real_solution(int64_t batch, int64_t num_loc, const int64_t* rec, int64_t* solution,
                         int32_t* status, void* stream);

/* TSPkoptEnv._reset after the initial solution (tsp/env.py:304-331) and get_costs
 * (base.py:361-369): cost[b] as defined above; visited_time (nullable, int64 [B, N]): the
 * walk from node 0 gives rec[0] the value 1, the next node 2, ... and node 0 the value N.
 * A rec that is not one N-cycle sets CO_ST_INVALID_TOUR; that row's outputs are
 * unspecified (nothing is written out of bounds). */
int co_tsp_kopt_reset(int64_t batch, int64_t num_loc, const float* locs, int64_t locs_batch,
                      const int64_t* rec, float* cost, int64_t* visited_time, int32_t* status,
                      void* stream);

/* TSPkoptEnv._step (tsp/env.py:259-302).  With `action` (element (b, a) at
 * action[b*act_stride_b + a*act_stride_a]): next_rec = operator(rec_in, action); with
 * action == NULL (step_to_solution): next_rec = rec_in, k_max is unused and i is not
 * touched.  Then
 *   rec_out = next_rec (in place over rec_in allowed); cost_current = cost(next_rec);
 *   cost_bsf_out = min(cost_current, cost_bsf_in) (in place allowed);
 *   reward = cost_bsf_in - cost_bsf_out; rows with reward > 0 overwrite their rec_best row
 *   (the reference mutates td["rec_best"] in place), the other rows of rec_best are left;
 *   visited_time as co_tsp_kopt_reset's; i_out = i_in + 1 (in place allowed).
 * Operator, k_max == 2 (DACT; action [B, 2] = (first, second), tsp/env.py:334-359): the
 * path first -> ... -> second is reversed: rec[pred(first)] = second, rec[first] =
 * rec_in[second] and every link inside the path turned round.  first == second changes
 * nothing; second == pred(first) reverses the whole tour (rec[first] = second).
 * Operator, k_max >= 3 (NeuOpt; action [B, 3*k_max] = index | left | right,
 * tsp/env.py:361-390), the reference's walk: rec_next = rec_in with rec_next[left[j]] =
 * right[j] for j = 0..k_max-1 in order (the last write wins); right_nodes =
 * rec_in[index[.]]; cur = left[0]; N - 2 times: next = rec_next[cur]; if pred(next) != cur
 * (pred of rec_in) and next is not in right_nodes: rec_next[next] = pred(next); cur = next.
 * An action entry outside 0..N-1 sets CO_ST_INDEX_RANGE; a rec_in or a result that is not
 * one N-cycle sets CO_ST_INVALID_TOUR; such a row's outputs are unspecified. */
int co_tsp_kopt_step(int64_t batch, int64_t num_loc, int64_t k_max, const float* locs,
                     int64_t locs_batch, const int64_t* rec_in, const int64_t* action,
                     int64_t act_stride_b, int64_t act_stride_a, int64_t* rec_out,
                     float* cost_current, const float* cost_bsf_in, float* cost_bsf_out,
                     float* reward, int64_t* rec_best, int64_t* visited_time,
                     const int64_t* i_in, int64_t* i_out, int32_t* status, void* stream);

/* `steps` consecutive co_tsp_kopt_step calls with preset actions in one launch: action
 * element (t, b, a) at actions[t*act_stride_t + b*act_stride_b + a*act_stride_a].  The
 * state is updated in place: rec_current, cost_bsf, rec_best, i (nullable; += steps), and
 * cost_current / visited_time are written for the last step (steps == 0: for the given
 * rec).  reward [steps, B] receives every step's reward, cost_steps (nullable,
 * [steps, B]) every step's cost_current.  Every output is bit-identical to the `steps`
 * single calls.  On the device the row's state stays in LDS between the steps: per step
 * the action is read and the reward written. */
int co_tsp_kopt_steps(int64_t batch, int64_t num_loc, int64_t k_max, int64_t steps,
                      const float* locs, int64_t locs_batch, const int64_t* actions,
                      int64_t act_stride_t, int64_t act_stride_b, int64_t act_stride_a,
                      int64_t* rec_current, float* cost_current, float* cost_bsf,
                      int64_t* rec_best, int64_t* visited_time, int64_t* i, float* reward,
                      float* cost_steps, int32_t* status, void* stream);

/* TSPGenerator._get_initial_solutions, "greedy" (tsp/generator.py:82-94): the
 * nearest-neighbour tour from node 0 as a linked list rec [B, N] (locs f32 [B, N, 2]).
 * Each step goes to the node with the smallest f32 distance D, a visited node counting as
 * 1e5 and the first minimum winning; the last node links back to 0. */
int co_tsp_nearest_rec(int64_t batch, int64_t num_loc, const float* locs, int64_t* rec,
                       void* stream);

/* ----------------------------------------------------------------- CVRP */

/* CVRPEnv._reset + get_action_mask (cvrp/env.py:107-149).  N = customers.
 * locs_out[B,N+1,2] = cat(depot[B,2], locs_in[B,N,2]); current_node[B,1] = 0;
 * used_capacity[B,1] = 0; vehicle_capacity_out[B,1] = vehicle_capacity;
 * visited[B,N+1] = 0; action_mask[B,N+1] per get_action_mask. */
int co_cvrp_reset(int64_t batch, int64_t num_loc, const float* depot, const float* locs_in,
                  const float* demand, float vehicle_capacity, float* locs_out,
                  int64_t* current_node, float* used_capacity, float* vehicle_capacity_out,
                  uint8_t* visited, uint8_t* action_mask, void* stream);

/* CVRPEnv._step fused with get_action_mask (cvrp/env.py:73-105,137-149):
 *   d = demand[b, clamp(a-1, 0, N-1)]; used_out = (used_in + d) * (a != 0)
 *   visited_out = visited_in with [a] = 1 (in-place allowed); current_out = a
 *   done = sum(visited_out) == N+1 ; reward = 0 (bool); action_mask recomputed.
 * not_done (optional) is atomically incremented by the number of rows not done
 * (the `while not td["done"].all()` poll of constructive/base.py:245 without a second
 * pass over `done`); the caller zeroes it. */
int co_cvrp_step(int64_t batch, int64_t num_loc, const int64_t* action, const float* demand,
                 const float* used_in, float* used_out, const float* vehicle_capacity,
                 const uint8_t* visited_in, uint8_t* visited_out, int64_t* current_out,
                 uint8_t* done, uint8_t* reward, uint8_t* action_mask, int32_t* status,
                 int32_t* not_done, void* stream);

/* CVRPEnv.get_action_mask alone (cvrp/env.py:137-149). current_node is [B,1]. */
int co_cvrp_action_mask(int64_t batch, int64_t num_loc, const float* demand, const float* used,
                        const float* vehicle_capacity, const uint8_t* visited,
                        const int64_t* current_node, uint8_t* action_mask, void* stream);

/* CVRPEnv.get_reward (cvrp/env.py:151-190): reward = -tour length of
 * [depot] + locs[actions] (closed).  check != 0 also runs
 * check_solution_validity: customers 1..N exactly once, every other entry 0
 * (CO_ST_INVALID_TOUR), then the per-step capacity scan
 * used = max(used + d, 0) <= vehicle_capacity + 1e-5 (CO_ST_OVER_CAPACITY). */
int co_cvrp_reward(int64_t batch, int64_t num_loc, int64_t steps, const float* locs,
                   const int64_t* actions, int64_t act_stride_b, int64_t act_stride_t,
                   const float* demand, const float* vehicle_capacity, int check, float* reward,
                   int32_t* status, void* stream);

/* Post-hoc improvement of CVRP rollouts: best-improvement 2-opt and relocate on the giant
 * tour of every row, the whole search of a row in one launch.  (The reference's
 * cvrp/local_search.py hands each instance to PyVRP with a randomised operator set and
 * growing load penalties; that is not reproduced.  This entry gives the capability: a
 * shorter, still feasible action matrix, deterministically.)
 *
 * Distances.  Exactly one of locs (f32 [LB, N+1, 2], depot first) and distances
 * (f32 [LB, N+1, N+1], row = first operand) is non-NULL; D[a, c] is distances[a, c] or the
 * f32 sqrt(dx*dx + dy*dy) co_distance_matrix writes (no FMA).  Row b uses instance b % LB
 * of locs / distances / demand [LB, N] / capacity [LB] (NULL = 1.0 for every row).
 *
 * Row check.  Every entry of the row (element (b, t) at actions[b*act_stride_b +
 * t*act_stride_t]) lies in 0..N, each of 1..N occurs exactly once, and each demand and the
 * capacity is finite and in [0, 4096]; otherwise the row is copied unchanged with 0 sweeps
 * and CO_ST_INVALID_TOUR is set.  A row that breaks capacity on input is not an error.
 *
 * Giant tour.  g[0] = 0, then the row's entries in order without a 0 that would follow a
 * 0, without a trailing 0; m = len(g) = N + the number of non-empty routes.  The tour is
 * cyclic (position m is position 0), g[0] never moves and m stays fixed: a route may
 * become empty, leaving two adjacent zeros.
 *
 * Loads.  q(x) = llrint((double)x * 2^40) in int64, so route loads are exact integer sums
 * and do not depend on order; cap_q = q(capacity) + 2^20.  (The generator's k / capacity
 * demands are rounded f32 values and routes that fill the vehicle exactly are common; the
 * slack of 9.5e-7 admits them and stays far inside the validity scan's 1e-5.)
 *
 * One sweep scores every candidate in f32, left to right as bracketed:
 *  - 2-opt (i, j), 1 <= i < j <= m-1: reverse g[i..j].  With p = g[i-1], x = g[i],
 *    y = g[j], n = g[(j+1) % m]:
 *      change = ((D[p,y] + D[x,n]) - D[p,x]) - D[y,n]
 *    (no skip test: reversing across a depot merges or re-cuts routes).  Admissible if
 *    g[i..j] holds no 0; otherwise both new boundary routes must have load <= cap_q:
 *    left = the customers of i-1's route at positions < i plus those after the last 0 of
 *    the segment up to j; right = the customers from i up to the first 0 of the segment
 *    plus those after j to the end of that route.  Routes wholly inside the segment are
 *    only reversed.
 *  - relocate (i, j), g[i] != 0, j in 0..m-1, j != i, j != i-1: customer c = g[i] moves
 *    to between positions j and j+1.  With p = g[i-1], n = g[(i+1) % m], a = g[j],
 *    b = g[(j+1) % m]:
 *      change = ((D[a,c] + D[c,b]) - D[a,b]) + ((D[p,n] - D[p,c]) - D[c,n])
 *    Admissible if gap j lies in c's own route (as many zeros in g[0..j] as in g[0..i]);
 *    otherwise the target route's load plus q(demand[c]) must be <= cap_q.
 * The smallest change among the admissible candidates with change < 0 is taken (equal
 * values: 2-opt before relocate, then the smaller i, then the smaller j) and applied when
 * it is < -1e-6 (compared in double): one move per sweep.  The search ends with the first
 * sweep that applies nothing or after max_iterations sweeps (<= 0: no sweep; above
 * 2^31 - 1 counts as 2^31 - 1).
 *
 * Output.  actions_out[batch, steps] (row-major; must not alias actions) receives the
 * routes of g in order, separated by single zeros, without a leading zero or empty routes,
 * padded with zeros to width steps -- a valid row with 0 sweeps comes back compacted.
 * sweeps_out[batch] (nullable) receives the sweeps executed.
 *
 * Limits: steps >= num_loc >= 1 and min(steps, 2*num_loc) + 1 <= CO_CVRP_LS_MAX_LEN, else
 * CO_E_INVAL.  One wavefront per row, tour state in LDS; a distances matrix of
 * num_loc <= CO_CVRP_LS_STAGE_N is staged in LDS, larger ones are read through L2. */
#define CO_CVRP_LS_MAX_LEN 1024
#define CO_CVRP_LS_STAGE_N 117
int co_cvrp_local_search(int64_t batch, int64_t num_loc, int64_t steps, const float* locs,
                         const float* distances, const float* demand, const float* capacity,
                         int64_t locs_batch, const int64_t* actions, int64_t act_stride_b,
                         int64_t act_stride_t, int64_t max_iterations, int64_t* actions_out,
                         int32_t* sweeps_out, int32_t* status, void* stream);

/* ----------------------------------------------------------------- SLAP */

/* SLAPEnv._reset (rl4co/envs/warehousing/slap/env.py:95-129). L = n_aisles*n_locs,
 * P = products: action_mask[B,L] = 1 except column 0 (depot); to_choose[B,P] =
 * 0..P-1 (float); i[B,1] = 0; reward[B,1] = 0; ratio[B,L] = 0 (ratio may be NULL); and
 * the zero done[B,1] / terminated[B,1] that RL4COEnvBase.reset adds (envs/common/base.py:
 * 138-143 via TorchRL; each may be NULL), so a reset is one launch. */
int co_slap_reset(int64_t batch, int64_t num_slots, int64_t n_products, uint8_t* action_mask,
                  float* to_choose, int64_t* i, float* reward, float* ratio, uint8_t* done,
                  uint8_t* terminated, void* stream);

/* SLAPEnv._step (slap/env.py:38-93): product p = (int)to_choose[b*tc_stride];
 * assign_out = assign_in with [b, p] = (int)action[b] (in-place allowed:
 * then only that element is written); mask_out = mask_in with [b, action] = 0
 * (in-place allowed); done[b] = (i_in[b] == P-1); reward[b] = 0 (bool);
 * i_out = i_in + 1.  Negative indices wrap like torch advanced indexing.
 * to_choose may be NULL when every row's to_choose[b, 0] holds one value k (the env's
 * untouched arange to_choose at step k, slap/env.py:105-108): tc_stride then carries k
 * (0 <= k < P) and no to_choose column is read (the same for co_slap_decode_step and
 * co_slap_closest_step). */
int co_slap_step(int64_t batch, int64_t num_slots, int64_t n_products, const int64_t* action,
                 const float* to_choose, int64_t tc_stride, const int32_t* assign_in,
                 int32_t* assign_out, const uint8_t* mask_in, uint8_t* mask_out,
                 const int64_t* i_in, int64_t* i_out, uint8_t* done, uint8_t* reward,
                 int32_t* status, void* stream);

/* SLAPEnv._get_reward (slap/env.py:131-143): for each order o (in order),
 * total -= closed Euclidean tour over locs[assignment[picklist[b, o, :]]]. */
int co_slap_reward(int64_t batch, int64_t num_slots, int64_t n_products, int64_t n_orders,
                   int64_t order_size, const int32_t* assignment, const int64_t* picklist,
                   const float* locs, float* reward, int32_t* status, void* stream);

/* Post-hoc improvement of SLAP assignments: best-improvement product swap + relocate, the
 * whole search of a row in one launch.  (The reference has no local search for SLAP;
 * SLAPEnv.local_search raises there.  The objective of slap/env.py:131-143 is a quadratic
 * assignment objective -- flow = how often product a is followed by product c in a
 * picklist, distance = slot to slot -- and this entry runs the classical QAP
 * neighbourhood on it, deterministically.)
 *
 * Inputs.  Exactly one of locs (f32 [LB, L, 2]) and distances (f32 [LB, L, L], row = first
 * operand, may be asymmetric) is non-NULL; D[u, v] is distances[u, v] or the f32
 * sqrt(dx*dx + dy*dy) co_distance_matrix writes (no FMA).  picklist is int64 [LB, O, K],
 * assignment int32 [B, P]: s[p] is the slot of product p.  Row b uses instance b % LB of
 * locs / distances / picklist (the un-replicated multistart layout).
 *
 * Objective, exact in integers.  Q[u][v] = llrint((double)D[u][v] * 2^20) in int64.
 * W[a][c] = the number of pairs (o, k) with picklist[o, k] = a, picklist[o, (k+1) % K] = c
 * and a != c (equal neighbours contribute nothing; W[a][c] <= O * (K / 2)).
 *   F(s) = sum over a, c of W[a][c] * Q[s[a]][s[c]]
 * With locs, F / 2^20 is -reward of co_slap_reward up to rounding.  Every sum is an exact
 * int64 (Q <= 2^40, a row of W sums to <= 2^16), so a candidate's change F(s') - F(s) does
 * not depend on how or in which order it is evaluated: the device's two evaluation
 * schemes, the host build and tests/slap_ls_ref.py are bit-equal.
 *
 * One sweep.  The candidates are
 *  - move (p, x): product p goes to slot x, 1 <= x <= L-1, x free (no product sits there).
 *    Slot 0 is the depot, which the env never offers (slap/env.py:116), so it is never a
 *    target; a product that already sits at slot 0 may leave it or be swapped.
 *  - swap (p, q), p < q: the two products exchange slots.
 * The candidate with the smallest change among those with change < 0 is applied, one per
 * sweep; equal changes: move before swap, then the smaller p, then the smaller x or q.
 * The search ends with the first sweep that applies nothing or after max_iterations sweeps
 * (<= 0: no sweep; above 2^31 - 1 counts as 2^31 - 1).  F strictly decreases, so it ends.
 *
 * Outputs.  assign_out [B, P] (must not alias assignment) receives the row;
 * sweeps_out [B] (nullable) the sweeps executed, the last one that applied nothing
 * included; cost_out [B] (nullable) F of the returned row.
 *
 * Row check.  Every s[p] lies in 0..L-1 and the slots are pairwise distinct (-1, the
 * unassigned product, is invalid); every picklist entry of the instance lies in 0..P-1
 * (no wrapping of negative entries); every coordinate of the instance is finite with
 * |coord| <= 2^18, or every entry of the instance's matrix is finite and in [0, 2^20].
 * A failing row is copied unchanged with 0 sweeps and cost_out = -1; it sets
 * CO_ST_INVALID_TOUR for an assignment or distance failure and CO_ST_INDEX_RANGE for a
 * picklist failure.
 *
 * Limits: 1 <= P <= CO_SLAP_LS_MAX_PRODUCTS, P <= L <= CO_SLAP_LS_MAX_SLOTS and
 * 1 <= O*K <= 65536, else CO_E_INVAL.
 *
 * Device.  One wavefront per row; W, s, the occupancy bitmap and the coordinates in LDS.
 * Two evaluation schemes with identical output: when it fits the LDS budget
 * (CO_SLAP_LS_TABLE_FITS(P, L): e.g. L <= 383 at P = 20, L <= 239 at P = 32, P = L <= 80)
 * the QAP table C[p][l] = sum over q of W[p][q]*Q[l][s[q]] + W[q][p]*Q[s[q]][l] is held in
 * LDS (a move costs C[p][x] - C[p][s[p]]; a swap two such differences and a
 * W[p][q] + W[q][p] term; an applied move updates O(P*L) entries); otherwise every
 * candidate is evaluated directly in O(P) terms.  A distances matrix is read through L2 by
 * both schemes (staging it in LDS was measured slower: DESIGN.md).
 * co_slap_local_search_scheme is the same entry with the scheme forced (CO_SLAP_LS_AUTO /
 * _DIRECT / _TABLE; _TABLE where the table does not fit is CO_E_INVAL): for tests and
 * measurements of one scheme against the other; device library only. */
#define CO_SLAP_LS_MAX_PRODUCTS 128
#define CO_SLAP_LS_MAX_SLOTS 1024
#define CO_SLAP_LS_LDS_BYTES 65536
/* an upper bound of the LDS bytes of a row's state without the table, and the table's cut */
#define CO_SLAP_LS_STATE_BYTES(P, L) (2 * (P) * ((P) + 1) + 4 * (P) + 8 * (L) + (L) / 8 + 64)
#define CO_SLAP_LS_TABLE_FITS(P, L) \
  (8 * (P) * (L) + CO_SLAP_LS_STATE_BYTES(P, L) <= CO_SLAP_LS_LDS_BYTES)
#define CO_SLAP_LS_AUTO 0
#define CO_SLAP_LS_DIRECT 1
#define CO_SLAP_LS_TABLE 2
int co_slap_local_search(int64_t batch, int64_t num_slots, int64_t n_products,
                         int64_t n_orders, int64_t order_size, const float* locs,
                         const float* distances, int64_t locs_batch, const int64_t* picklist,
                         const int32_t* assignment, int64_t max_iterations, int32_t* assign_out,
                         int32_t* sweeps_out, int64_t* cost_out, int32_t* status, void* stream);
int co_slap_local_search_scheme(int64_t batch, int64_t num_slots, int64_t n_products,
                                int64_t n_orders, int64_t order_size, const float* locs,
                                const float* distances, int64_t locs_batch,
                                const int64_t* picklist, const int32_t* assignment,
                                int64_t max_iterations, int32_t* assign_out,
                                int32_t* sweeps_out, int64_t* cost_out, int32_t scheme,
                                int32_t* status, void* stream);

/* ------------------------------------------------------------ utilities */

/* utils.ops.gather_by_index (rl4co/utils/ops.py:65-77), gather along one dim:
 * src element (o, j, :) at src + o*src_stride_outer + j*src_stride_len (bytes),
 * `inner_bytes` contiguous bytes each; idx (o, m) at idx[o*idx_stride_outer +
 * m*idx_stride_len]; dst[o, m, :] contiguous [outer, idx_len, inner_bytes].
 * Out-of-range index: CO_ST_INDEX_RANGE and a zero-filled output element. */
int co_gather_by_index(const void* src, int64_t outer, int64_t src_len, int64_t inner_bytes,
                       int64_t src_stride_outer, int64_t src_stride_len, const int64_t* idx,
                       int64_t idx_len, int64_t idx_stride_outer, int64_t idx_stride_len,
                       void* dst, int32_t* status, void* stream);

/* The batch-wide test of tsp/env.py:70: *flag = any(x[0..n) == value). */
int co_any_eq_i64(const int64_t* x, int64_t n, int64_t value, int32_t* flag, void* stream);

/* ---------------------------------------------------------- decode step */

#define CO_DECODE_GREEDY 0
#define CO_DECODE_SAMPLING 1
#define CO_DECODE_EVALUATE 2
/* mode flag (OR-ed into `mode`), opt-in: hardware v_exp tanh / exp and lane-order sums.
 * Without it the step is ATen-exact: logp bit-identical to F.log_softmax of the processed
 * logits (SLEEF expf/logf and vec::map_reduce_all's 16-lane order), tanh correctly
 * rounded; with it logp is within ~1e-6 and greedy picks may differ on near-ties. */
#define CO_DECODE_FAST 0x100
/* mode flag, opt-in: greedy picks computed with the fast math and certified per row by
 * its error bound (the runner-up must trail the pick by more than the fast tanh error
 * times the clip plus two ulps of the log-sum-exp); any wave holding an uncertified row
 * is recomputed with the exact math.  Greedy actions are therefore the exact path's;
 * the selected logp is the fast one (within ~1e-6).  Other modes run exact under it. */
#define CO_DECODE_CERTIFIED 0x200

/* DecodingStrategy.step (rl4co/utils/decoding.py:141-191,327-399,489-499):
 * x = logits[b*logits_stride + c]; tanh clip (tanh_clipping > 0); masked
 * (mask != NULL and mask[b*n+c] == 0) -> -inf; x /= temperature;
 * logp = (x - max) - log(sum(exp(x - max))) (ATen's CPU evaluation, bit-exact; see
 * CO_DECODE_FAST);
 * greedy: first argmax of logp (torch tie-break); sampling: inverse CDF of
 * exp(logp) with a Philox draw keyed by (seed, offset, b); evaluate: action_in.
 * action_out[b], logp_sel[b] = logp[b, action]; logprobs_full (nullable)
 * receives the whole row.  Greedy/sampling picking a masked action sets
 * CO_ST_INFEASIBLE.  Rows of n_actions > 2048 run a workgroup-per-row kernel in the
 * exact math whatever the math flags (top-p filtering is not offered there: CO_E_INVAL). */
int co_decode_step(int64_t batch, int64_t n_actions, const float* logits, int64_t logits_stride,
                   const uint8_t* mask, float tanh_clipping, float temperature, int mode,
                   const int64_t* action_in, int64_t* action_out, float* logp_sel,
                   float* logprobs_full, uint64_t seed, uint64_t offset, int32_t* status,
                   void* stream);

/* co_decode_step with the top-k / top-p filters of process_logits (decoding.py:112-138,
 * 183-187) applied after the temperature: top_k > 0 keeps values >= the k-th largest
 * (torch.topk, multiplicity counted); 0 < top_p < 1 drops elements whose ascending
 * cumulative softmax probability (ties by index) is <= 1 - top_p.  top_k = 0 / top_p = 0
 * disable them (co_decode_step == this with 0, 0). */
int co_decode_step_ex(int64_t batch, int64_t n_actions, const float* logits,
                      int64_t logits_row_stride, const uint8_t* mask, float tanh_clipping,
                      float temperature, int top_k, double top_p, int mode,
                      const int64_t* action_in, int64_t* action_out, float* logp_selected,
                      float* logp_full, uint64_t seed, uint64_t offset, int32_t* status,
                      void* stream);

/* co_decode_step fused with TSPEnv._step (tsp/env.py:67-93) for the selected action:
 * mask_out = mask_in minus the action (in-place NOT allowed), i_out = i_in + 1,
 * first_out = first_mode ? action : first_in, done = nothing left, step_reward = 0,
 * action_out / logp_sel as co_decode_step (action_out must not alias action_in);
 * ll_accum (nullable) += logp_sel: get_log_likelihood's sum (decoding.py:39-65).
 * The decode-fused env-step of SURVEY.md 8d (4N + 4 B on top of co_tsp_step). */
int co_tsp_decode_step(int64_t batch, int64_t num_loc, const float* logits,
                       int64_t logits_stride, const uint8_t* mask_in, float tanh_clipping,
                       float temperature, int mode, const int64_t* action_in,
                       int64_t* action_out, float* logp_sel, uint64_t seed, uint64_t offset,
                       uint8_t* mask_out, const int64_t* i_in, int64_t* i_out,
                       const int64_t* first_in, int64_t* first_out, int first_mode,
                       uint8_t* done, uint8_t* step_reward, float* ll_accum, int32_t* status,
                       void* stream);

/* co_decode_step fused with SLAPEnv._step (slap/env.py:38-93) for the selected action
 * (replaces DecodingStrategy.step + env.step of constructive/base.py:245-251 on the fork's
 * examples/slap.py policy path).  L = locations (the row length of logits / masks),
 * P = products.  Decode as co_decode_step; then, with a = the selected action (evaluate:
 * action_in, negative values index from the end as python indexing):
 *   assign_out = assign_in with [b, (int)to_choose[b*tc_stride]] = (int)a (out of place:
 *   the row is copied; in place: that element only); mask_out = mask_in minus a
 *   (in place allowed, as i_out = i_in); done[b] = i_in[b] == P-1; i_out = i_in + 1; step_reward = 0;
 *   ll_accum (nullable) += logp_sel.  Same bits as co_decode_step + co_slap_step. */
int co_slap_decode_step(int64_t batch, int64_t num_slots, int64_t n_products,
                        const float* logits, int64_t logits_stride, const uint8_t* mask_in,
                        float tanh_clipping, float temperature, int mode,
                        const int64_t* action_in, int64_t* action_out, float* logp_sel,
                        uint64_t seed, uint64_t offset, const float* to_choose,
                        int64_t tc_stride, const int32_t* assign_in, int32_t* assign_out,
                        uint8_t* mask_out, const int64_t* i_in, int64_t* i_out, uint8_t* done,
                        uint8_t* step_reward, float* ll_accum, int32_t* status, void* stream);

/* co_decode_step fused with CVRPEnv._step + get_action_mask (cvrp/env.py:73-149):
 * N = customers, rows of logits / masks / visited are N+1 wide.  Decode as
 * co_decode_step; then the co_cvrp_step transition for the selected action (evaluate:
 * action_in): used_out, visited_out (separate buffer), current_out (nullable) = a,
 * done, step_reward = 0, action_mask recomputed into mask_out (separate buffer);
 * ll_accum (nullable) += logp_sel.  Same bits as co_decode_step + co_cvrp_step. */
int co_cvrp_decode_step(int64_t batch, int64_t num_loc, const float* logits,
                        int64_t logits_stride, const uint8_t* mask_in, float tanh_clipping,
                        float temperature, int mode, const int64_t* action_in,
                        int64_t* action_out, float* logp_sel, uint64_t seed, uint64_t offset,
                        const float* demand, const float* used_in, float* used_out,
                        const float* vehicle_capacity, const uint8_t* visited_in,
                        uint8_t* visited_out, int64_t* current_out, uint8_t* done,
                        uint8_t* step_reward, uint8_t* mask_out, float* ll_accum,
                        int32_t* status, void* stream);

/* ------------------------------------------- bench policies (in-kernel) */

/* Deterministic cheap policies for the env-throughput benchmark
 * (SURVEY.md 8d); they are the "policy" half of a rollout, not reference code.
 * TSP: step0 -> 0, then nearest unvisited to current_node (ties lowest index).
 * CVRP: nearest feasible customer, else depot.  SLAP: free location with the
 * lowest depot_loc_dist.  first_step != 0 selects the TSP step-0 branch, which reads
 * none of locs / action_mask / current_node (they may be NULL then).  locs is read as
 * (x, y) pairs and must be 8-byte aligned wherever it is read: CO_E_ALIGN otherwise, for
 * all of co_tsp_nearest_action (first_step == 0), co_cvrp_nearest_action and
 * co_cvrp_nearest_step. */
int co_tsp_nearest_action(int64_t batch, int64_t num_loc, const float* locs,
                          const uint8_t* action_mask, const int64_t* current_node, int first_step,
                          int64_t* action_out, void* stream);
int co_cvrp_nearest_action(int64_t batch, int64_t num_loc, const float* locs,
                           const uint8_t* action_mask, const int64_t* current_node,
                           int64_t* action_out, void* stream);
int co_slap_closest_free_action(int64_t batch, int64_t num_slots, const float* depot_loc_dist,
                                const uint8_t* action_mask, int64_t* action_out, void* stream);
/* The nearest-feasible bench policy fused with CVRPEnv._step + get_action_mask
 * (cvrp/env.py:73-149): the action co_cvrp_nearest_action would pick from (mask_in,
 * cur_in) is written to action_out and applied as co_cvrp_step does, in one launch.
 * In place (visited_out == visited_in, mask_out == mask_in) is allowed.  Results are
 * identical to the two calls (which it falls back to for N + 1 > 128). */
int co_cvrp_nearest_step(int64_t batch, int64_t num_loc, const float* locs, const float* demand,
                         const float* used_in, float* used_out, const float* vehicle_capacity,
                         const uint8_t* visited_in, uint8_t* visited_out,
                         const uint8_t* mask_in, const int64_t* current_in, int64_t* action_out,
                         int64_t* current_out, uint8_t* done, uint8_t* reward, uint8_t* mask_out,
                         int32_t* status, int32_t* not_done, void* stream);
/* The closest-free bench policy fused with SLAPEnv._step (slap/env.py:38-93): the
 * action co_slap_closest_free_action would pick is written to action_out and applied
 * as co_slap_step does (assign_out = assign_in with [b, p] = action; in-place allowed),
 * in one launch.  Results identical to the two calls (which it falls back to when
 * num_slots % 4 != 0, num_slots > 256 or the buffers are misaligned). */
int co_slap_closest_step(int64_t batch, int64_t num_slots, int64_t n_products,
                         const float* depot_loc_dist, const float* to_choose, int64_t tc_stride,
                         const int32_t* assign_in, int32_t* assign_out, const uint8_t* mask_in,
                         uint8_t* mask_out,
                         int64_t* action_out, const int64_t* i_in, int64_t* i_out, uint8_t* done,
                         uint8_t* reward, int32_t* status, void* stream);

/* K consecutive co_slap_closest_step calls in one launch (round 6): the state ping-pongs
 * between buffers A and B (step k reads mask / i from A for even k, from B for odd k, and
 * writes the other), step k's action to action_out + k*act_stride, its product from
 * to_choose column k (row stride tc_stride; with to_choose NULL the uniform product
 * tc_stride + k), the assignment of step 0 written out of place from assign_in when it
 * differs from assign_out and in place after; done / reward written by every step.  Each
 * step stores its whole state as its own launch would; the final contents are
 * bit-identical to the K calls.  For the stepwise engine's closest-free bench policy. */
int co_slap_closest_steps(int64_t batch, int64_t num_slots, int64_t n_products, int64_t steps,
                          const float* depot_loc_dist, const float* to_choose, int64_t tc_stride,
                          const int32_t* assign_in, int32_t* assign_out, uint8_t* mask_a,
                          int64_t* i_a, uint8_t* mask_b, int64_t* i_b, int64_t* action_out,
                          int64_t act_stride, uint8_t* done, uint8_t* reward, int32_t* status,
                          void* stream);

/* -------------------------------------------- fused episode rollouts */

/* One launch per episode (reset + N steps + reward) for the env-only rollout of
 * rl4co/utils/decoding.py:88-109 with the policy in-kernel.  Each step applies
 * TSPEnv._step (tsp/env.py:67-93) to register state; only what a caller can
 * observe after rollout() is written: the final action_mask[B,N], first_node[B],
 * current_node[B], i[B,1] (= N), done[B], the last step's bool reward[B], the
 * episode reward[B] (= -closed tour length, TSPEnv.get_reward) and, for the
 * in-kernel policy, the actions.  Actions are step-major [N, B] (row t = the [B]
 * action tensor of step t).  acts_in != NULL: teacher-forced (Evaluate mode);
 * acts_in == NULL: nearest-unvisited policy (co_tsp_nearest_action) writing
 * acts_out.  check != 0: a non-permutation sets CO_ST_INVALID_TOUR.  One launch for
 * N <= 256 (teacher) / N <= 1024 (nearest); longer episodes run the same steps as a
 * sequence of the stepwise kernels (co_tsp_reset, co_tsp_step in place, co_tsp_reward),
 * with identical outputs. */
int co_tsp_rollout(int64_t batch, int64_t num_loc, const float* locs, const int64_t* acts_in,
                   int64_t* acts_out, uint8_t* action_mask, int64_t* first_node,
                   int64_t* current_node, int64_t* i, uint8_t* done, uint8_t* step_reward,
                   float* reward, int check, int32_t* status, void* stream);

/* co_tsp_rollout with the teacher actions' layout given by strides: element (b, t) at
 * acts_in[b*act_stride_b + t*act_stride_t].  (1, batch) is co_tsp_rollout's step-major
 * [N, B]; (>= num_loc, 1) is row-major [B, N] -- the reference's [B, T] layout
 * (ConstructivePolicy's `actions`, rl4co/models/common/constructive/base.py:223-230): one
 * lane group per instance reads the instance's contiguous action and coordinate rows
 * (num_loc <= 1024).  acts_in == NULL: the nearest policy as co_tsp_rollout (strides
 * unused).  Same outputs as co_tsp_rollout. */
int co_tsp_rollout_ex(int64_t batch, int64_t num_loc, const float* locs, const int64_t* acts_in,
                      int64_t act_stride_b, int64_t act_stride_t, int64_t* acts_out,
                      uint8_t* action_mask, int64_t* first_node, int64_t* current_node,
                      int64_t* i, uint8_t* done, uint8_t* step_reward, float* reward, int check,
                      int32_t* status, void* stream);

/* CVRP episode in one launch (cvrp/env.py:73-190 under decoding.py:88-109 rollout):
 * reset from the generator columns (depot[B,2], locs[B,N,2], demand[B,N] already
 * divided by the capacity, vehicle capacity vcap), then the nearest-feasible policy
 * (co_cvrp_nearest_action's rule) until every instance is done, then the closed-tour
 * reward.  Actions are step-major [max_steps, B]; *steps_out (device int32) receives
 * the batch-wide episode length T (the reference's number of loop iterations); rows
 * [len_b, T) of a shorter episode hold the depot steps the reference applies to
 * finished instances, and their state reflects them.  Writes locs_out[B,N+1,2]
 * (nullable), current_node[B], used_capacity[B], vehicle_capacity[B], visited[B,N+1],
 * action_mask[B,N+1], done[B], step_reward[B] (bool 0), reward[B], len_out[B] (own
 * episode length).  An instance not done after max_steps sets CO_ST_TRUNCATED.
 * N <= 1023. */
int co_cvrp_rollout(int64_t batch, int64_t num_loc, const float* depot, const float* locs,
                    const float* demand, float vehicle_capacity, int64_t max_steps,
                    int64_t* acts_out, float* locs_out, int64_t* current_node,
                    float* used_capacity, float* vehicle_capacity_out, uint8_t* visited,
                    uint8_t* action_mask, uint8_t* done, uint8_t* step_reward, float* reward,
                    int32_t* len_out, int32_t* steps_out, int32_t* status, void* stream);

/* SLAP episode in one launch (slap/env.py:38-143): P steps (product t <- the
 * step-t location; locations masked; done at i == P-1) then the per-order pick
 * tour reward.  Writes action_mask[B,L], assignment[B,P] (from assign_in, the
 * generator's -1s), i[B,1] (= P), done[B,1], step_reward[B,1], reward[B] and
 * ratio[B,L] = 0 (nullable).  acts_in != NULL: teacher-forced step-major [P,B];
 * acts_in == NULL: closest-free policy on depot_dist, written to acts_out.  L <= 256. */
int co_slap_rollout(int64_t batch, int64_t num_slots, int64_t n_products, int64_t n_orders,
                    int64_t order_size, const float* locs, const int64_t* picklist,
                    const float* depot_dist, const int32_t* assign_in, const int64_t* acts_in,
                    int64_t* acts_out, uint8_t* action_mask, int32_t* assignment, int64_t* i,
                    uint8_t* done, uint8_t* step_reward, float* reward, float* ratio,
                    int32_t* status, void* stream);

/* POMO shared baseline (rl4co/models/rl/reinforce/baselines.py:57-61,
 * reinforce.py:97-115, zoo/pomo/model.py:105-114) over the multistart layout
 * env e = s*instances + b: bl[b] = mean_s reward, max_reward[b] / best_start[b] =
 * max / first argmax over s, adv[e] = reward[e] - bl[b] and
 * loss_terms[b] = sum_s adv * log_likelihood (loss = -sum_b loss_terms / (S*B)).
 * log_likelihood / adv / loss_terms may be NULL. */
int co_pomo_shared_baseline(int64_t instances, int64_t starts, const float* reward,
                            const float* log_likelihood, float* bl, float* max_reward,
                            int64_t* best_start, float* adv, float* loss_terms, void* stream);

/* ------------------------------------------------ policy evaluation (rl4co/tasks/eval.py)
 * The K-candidate evaluators (augmentations x starts x samples, eval.py:129-144,220-238,
 * 278-301) score K*B action rows, unbatchify, take max(dim=1) and gather the winners.
 * The candidate layout is batchify's repeat-major one: candidate k of instance b is row
 * e = k*B + b (B = instances, K = candidates).
 *
 * Segmented best-of-K: best_idx[b] = the k whose reward[k*B + b] is largest (equal values,
 * +0/-0 included: the lowest k; a NaN beats every number and the first NaN wins, as
 * torch.max(dim) does); best_reward[b] = that value; best_actions[b, 0..T-1] (row-major,
 * nullable) = that candidate's action row.  Action element (e, t) at
 * actions[e*act_stride_b + t*act_stride_t].  best_actions must not alias actions; status
 * is unused (the selection has no data-dependent failure) and may be NULL. */
int co_best_of(int64_t instances, int64_t candidates, int64_t steps, const float* reward,
               const int64_t* actions, int64_t act_stride_b, int64_t act_stride_t,
               float* best_reward, int64_t* best_idx, int64_t* best_actions,
               int32_t* status, void* stream);

/* The same selection fused with TSPEnv.get_reward on the UN-replicated instances:
 * locs f32 [instances, num_loc, 2]; every candidate row is a tour of T = num_loc steps
 * (num_loc <= 1024, else CO_E_INVAL).  A candidate's reward is co_tsp_reward's: the
 * negated f32 rounding of a double sum of the f32 edge lengths of the closed tour (the
 * summation order is not fixed: a value may differ from co_tsp_reward's by one f32 ulp);
 * the selection is exact on these values.  all_reward (nullable, f32 [K*B]) receives
 * every candidate's reward.  check != 0: any candidate row that is not a permutation sets
 * CO_ST_INVALID_TOUR (winner or not); an out-of-range index sets CO_ST_INDEX_RANGE as
 * co_tsp_reward does.  best_actions (nullable, [instances, num_loc]) must not alias
 * actions.  One launch: the instance's coordinates are read once for its K candidates. */
int co_tsp_best_of(int64_t instances, int64_t num_loc, int64_t candidates, const float* locs,
                   const int64_t* actions, int64_t act_stride_b, int64_t act_stride_t,
                   int check, float* all_reward, float* best_reward, int64_t* best_idx,
                   int64_t* best_actions, int32_t* status, void* stream);

/* The deterministic part of SLAPGenerator._generate (slap/generator.py:51-81,137-155):
 * locs[B,L,2] aisle grid (x = aisle * inter_aisle_dist, y = loc * inter_loc_dist, products
 * in double rounded to f32), depot_loc_dist[B,L] and dist_mat[B,L,L] (nullable;
 * Manhattan, f32) and assignment[B,P] = -1 (nullable); L = n_aisles * n_locs.  freq and
 * the picklists stay on the host RNG streams. */
int co_slap_generate(int64_t batch, int64_t n_aisles, int64_t n_locs, double inter_aisle_dist,
                     double inter_loc_dist, int64_t n_products, float* locs,
                     float* depot_loc_dist, float* dist_mat, int32_t* assignment,
                     void* stream);

/* dihedral_8_augmentation (rl4co/data/transforms.py:15-37): out[8B, N, 2], row r*B + b
 * = transform r of instance b, r in the reference's order (x,y) (1-x,y) (x,1-y)
 * (1-x,1-y) (y,x) (1-y,x) (y,1-x) (1-y,1-x). */
int co_dihedral8_augment(int64_t batch, int64_t num_loc, const float* xy, float* out,
                         void* stream);

/* symmetric_transform (rl4co/data/transforms.py:49-71) given the per-row angles phi[B]
 * (drawn by the caller exactly as symmetric_augmentation does, transforms.py:74-93):
 * rotate (x,y) - offset by phi, swap the axes where phi > 2*pi, add the offset. */
int co_symmetric_augment(int64_t batch, int64_t num_loc, const float* xy, const float* phi,
                         float offset, float* out, void* stream);

/* BeamSearch._make_beam_step (rl4co/utils/decoding.py:611-641): rows e = s*B + b of
 * logp[BW*B, N] (full log-probabilities of the beams) plus parent[e] are ranked per
 * instance over the BW*N (beam, node) candidates; the BW best (descending; equal scores
 * -> lower candidate index s*N + c) are written to rows j*B + b: selected node,
 * beam_parent s, beam_row = b + s*B (the state row to continue from) and the new parent
 * score.  mask != NULL: a selected node with mask 0 sets CO_ST_INFEASIBLE
 * (decoding.py:519-522).  BW*N <= 36864. */
int co_beam_select(int64_t batch, int64_t beam_width, int64_t n_actions, const float* logp,
                   int64_t logp_row_stride, const float* parent, const uint8_t* mask,
                   int64_t* selected, int32_t* beam_parent, int64_t* beam_row,
                   float* score_out, int32_t* status, void* stream);

/* get_distance_matrix (rl4co/utils/ops.py:104-111): out[B, N, N] = Euclidean distances
 * between the instance's coordinates, f32 sqrt(dx*dx + dy*dy).  out 16-byte aligned. */
int co_distance_matrix(int64_t batch, int64_t num_loc, const float* locs, float* out,
                       void* stream);

/* Number of rows with done[b] == 0 written to *count (device int32). */
int co_count_not_done(const uint8_t* done, int64_t n, int32_t* count, void* stream);

/* *out (device int32) = max(0, max over rows b of (width - sum of rows[b*row_stride + c],
 * c < width)).  The decode loop's `while not td["done"].all()` poll for CVRP
 * (constructive/base.py:245, cvrp/env.py:92 done = visited.sum(-1) == N+1): a positive
 * deficit d means no instance set can be all done within the next d - 1 steps, so those
 * host syncs are skipped without changing the stopping step. */
int co_row_deficit_max(const uint8_t* rows, int64_t n_rows, int64_t width, int64_t row_stride,
                       int32_t* out, void* stream);

/* Device instance generation for throughput runs: the Uniform
 * samplers of tsp/generator.py:51-60 and cvrp/generator.py:116-143 on a Philox-4x32-10
 * stream (key = seed, block counter offset + i/4) instead of torch's CPU generator, so the
 * values follow torch's f32 uniform grid and transform but not its stream (parity
 * instances keep the host generators).  demand == 0: out[i] = low + u*(high-low);
 * demand != 0: out[i] = ((int)(low + u*(high-low)) + 1) / capacity. */
int co_uniform_fill(float* out, int64_t n, float low, float high, float capacity, int demand,
                    uint64_t seed, uint64_t offset, void* stream);

/* Integers in [low, high) on the same Philox stream layout, for SLAP picklists in
 * throughput runs (slap/generator.py:137-155 draws them with numpy's randint):
 * out[i] = low + ((uint64)x_i * (high - low)) >> 32, 0 < high - low < 2^32. */
int co_randint_fill(int64_t* out, int64_t n, int64_t low, int64_t high, uint64_t seed,
                    uint64_t offset, void* stream);

/* ------------------------------------------------ measurement utility (no reference
 * counterpart): dst[0:nbytes) = src[0:nbytes), one 16-byte load/store per thread over a
 * full grid -- the streaming ceiling the bench quotes beside each kernel's roofline.
 * src/dst 16-byte aligned, nbytes a multiple of 16. */
int co_probe_copy(const void* src, void* dst, int64_t nbytes, void* stream);

/* The decode loop's epilogue (DecodingStrategy.post_decoder_hook, decoding.py:315-325, and
 * get_log_likelihood, decoding.py:39-65) in one launch.  The T per-step [B] actions and
 * log-probabilities are rows of step-major slabs (act_sm[t * act_rs + b], logp_sm[t *
 * logp_rs + b]: the tensors the per-step calls returned); writes torch.stack(..., 1) =
 * actions[B, T] / logprobs[B, T], ll[B] = logprobs.sum(1) (summed in step order in f64,
 * rounded once; may be NULL), and ORs CO_ST_LOGP_NEG_INF into status when any log-
 * probability is not > -1000 (the assert of decoding.py:57-58).  act_sm or logp_sm may be
 * NULL (that half is skipped). */
int co_episode_stack(int64_t batch, int64_t steps, const int64_t* act_sm, int64_t act_rs,
                     const float* logp_sm, int64_t logp_rs, int64_t* actions, float* logprobs,
                     float* ll, int32_t* status, void* stream);

/* --------------------------------------------------------------- CVRPTW */

/* CVRP with time windows (rl4co/envs/routing/cvrptw/env.py).  N = customers, NC = N + 1
 * columns (the depot first), 1 <= N <= CO_CVRPTW_MAX_N, else CO_E_INVAL; an empty batch is
 * a no-op; a NULL pointer not marked nullable is CO_E_INVAL.
 *
 * Dtypes.  `durations` [B, NC] and `time_windows` [B, NC, 2] (start, end) arrive in the
 * td's own dtype with a code CO_DT_* (the generator gives f32 durations and i32 windows,
 * f32 windows with scale=True; extract_from_solomon gives i64 for both); an unknown code is
 * CO_E_MODE.  Every value is converted with a plain cast to f32 on load, which is torch's
 * promotion of an integer tensor meeting the f32 current_time / distances.
 *
 * Distance.  dist(p, q) = sqrtf(dx*dx + dy*dy), dx = p.x - q.x, dy = p.y - q.y, in f32,
 * every operation rounded on its own (no FMA), sqrtf correctly rounded: the value
 * co_distance_matrix writes.  This is the product's formula and is NOT bit-equal to
 * torch's CPU norm(p=2) (get_distance, utils/ops.py): over random legs in [0, 150]^2 about
 * 8 % differ, each by one ulp.
 *
 * The mask of a state (get_action_mask, env.py:103-115), c = 0..N:
 *   current_loc  = locs[b, clamp(current_node, 0, N)]
 *   distances[c] = dist(current_loc, locs[b, c])
 *   cvrp[c]      = co_cvrp_action_mask's value: a customer is open when not visited and
 *                  not (demand[c-1] + used > vehicle_capacity); the depot is open unless
 *                  (current_node == 0 and some customer is open) -- "open" before the time
 *                  test, as the reference computes the depot column from the CVRP mask
 *   action_mask[c] = cvrp[c] && (current_time + distances[c] <= (f32)time_windows[c][1])
 * The deadline test is f32, applies to the depot column too, and is false for a NaN.
 *
 * The step (env.py:117-134), a = action[b], ac = clamp(a, 0, N); a outside 0..N sets
 * CO_ST_INDEX_RANGE and leaves `visited` unchanged, as co_cvrp_step does:
 *   x = max(current_time_in + distances_in[b, ac], (f32)time_windows[ac][0])
 *       (torch.max: NaN when either operand is NaN) + (f32)durations[ac]
 *   current_time = (float)(a != 0) * x              (so 0 * NaN stays NaN)
 *   then co_cvrp_step's sequence unchanged (used = (used + d) * (float)(a != 0), visited,
 *   current_node = a, done = sum(visited) == NC, reward = 0), then the mask above on the
 *   new state.  distances_in is the vector the previous mask call left in the td. */
#define CO_CVRPTW_MAX_N 1023
#define CO_DT_F32 0
#define CO_DT_I32 1
#define CO_DT_I64 2

/* status bits of co_cvrptw_check, one per message of check_solution_validity
 * (cvrptw/env.py:172-218), in the reference's order */
#define CO_ST_TW_NEGATIVE 64          /* "Time windows must be non-negative."       :182 */
#define CO_ST_TW_DEPOT_RETURN 128     /* "vehicle cannot perform service and get back to
                                         depot in time."                            :183-186 */
#define CO_ST_DURATION_NEGATIVE 256   /* "Service durations must be non-negative."  :187-189 */
#define CO_ST_TW_INFEASIBLE 512       /* "there are unfeasible time windows"        :190-192 */
#define CO_ST_TW_DEADLINE 1024        /* "vehicle cannot start service before deadline" :208-213 */

/* CVRPTWEnv._reset (env.py:136-165) in one launch: co_cvrp_reset's outputs plus
 * current_time[B,1] = 0, current_loc[B,2] = depot, distances[B,NC] and the mask above. */
int co_cvrptw_reset(int64_t batch, int64_t num_loc, const float* depot, const float* locs_in,
                    const float* demand, float vehicle_capacity, const void* time_windows,
                    int tw_dtype, float* locs_out, int64_t* current_node, float* current_time,
                    float* used_capacity, float* vehicle_capacity_out, uint8_t* visited,
                    float* current_loc, float* distances, uint8_t* action_mask, void* stream);

/* CVRPTWEnv._step (env.py:117-134) in one launch: the time update, CVRP's step and the new
 * mask, as stated above.  locs is the post-reset [B, NC, 2].  visited_out may be visited_in
 * (in-place allowed); every other output is a buffer of its own.  status / not_done
 * (nullable) as in co_cvrp_step.  One step moves 27 N + 77 bytes per row with i32 / f32
 * windows (locs 8 NC, windows 8 NC, demand 4 N, visited NC in and NC out, distances 4 NC
 * and the mask NC out, 54 bytes of row scalars; i64 windows: 8 NC more), about 2.8 KB at
 * N = 100, against NC square roots: the kernel is bandwidth-bound. */
int co_cvrptw_step(int64_t batch, int64_t num_loc, const int64_t* action, const float* locs,
                   const float* demand, const float* used_in, float* used_out,
                   const float* vehicle_capacity, const uint8_t* visited_in,
                   uint8_t* visited_out, const float* current_time_in,
                   const float* distances_in, const void* durations, int dur_dtype,
                   const void* time_windows, int tw_dtype, float* current_time_out,
                   int64_t* current_out, uint8_t* done, uint8_t* reward, float* current_loc,
                   float* distances, uint8_t* action_mask, int32_t* status, int32_t* not_done,
                   void* stream);

/* CVRPTWEnv.get_action_mask alone (env.py:103-115); also writes current_loc [B,2] and
 * distances [B,NC], which the reference stores in the td.  current_node / current_time are
 * [B,1]. */
int co_cvrptw_action_mask(int64_t batch, int64_t num_loc, const float* locs, const float* demand,
                          const float* used, const float* vehicle_capacity,
                          const uint8_t* visited, const int64_t* current_node,
                          const float* current_time, const void* time_windows, int tw_dtype,
                          float* current_loc, float* distances, uint8_t* action_mask,
                          void* stream);

/* The time-window part of check_solution_validity (env.py:176-218; CVRP's part is
 * co_cvrp_reward with check != 0) for actions [B, T] (element (b, t) at b*act_stride_b +
 * t*act_stride_t).  With tw = (f32)time_windows, dur = (f32)durations, d0[c] = dist(locs[b,
 * 0], locs[b, c]), per row and column:
 *   tw < 0 (either end)                                       CO_ST_TW_NEGATIVE
 *   !((tw[c][0] + d0[c]) + dur[c] <= tw[0][0][1])             CO_ST_TW_DEPOT_RETURN
 *       -- the bound is the depot deadline OF BATCH ROW 0, as in the reference, read on
 *       the device (no host sync)
 *   dur[c] < 0                                                CO_ST_DURATION_NEGATIVE
 *   !(tw[c][0] < tw[c][1])                                    CO_ST_TW_INFEASIBLE
 * then the scan from t = 0 at the depot, per action a (out of 0..N: CO_ST_INDEX_RANGE, the
 * row's scan ends):
 *   t = max(trunc(t + dist(locs[prev], locs[a])), tw[a][0]); !(t <= tw[a][1]) sets
 *   CO_ST_TW_DEADLINE; t += dur[a]; t = 0 when a == 0.
 * trunc is the reference's `.int()`: toward zero, and -2^31 for a NaN or a value outside
 * int32 (what the x86 conversion gives).  All of it in f32 (integer windows below 2^24 are
 * exact).  The reference's "Distances must be non-negative." (:181) cannot fail for finite
 * coordinates -- a square root is never negative -- and has no bit. */
int co_cvrptw_check(int64_t batch, int64_t num_loc, int64_t steps, const float* locs,
                    const int64_t* actions, int64_t act_stride_b, int64_t act_stride_t,
                    const void* durations, int dur_dtype, const void* time_windows,
                    int tw_dtype, int32_t* status, void* stream);

/* `steps` (>= 1) preset co_cvrptw_step calls in one launch: action (t, b) at
 * actions[t*act_stride_t + b*act_stride_b].  used / visited / current_time / current_node
 * are updated in place ([B,1] / [B,NC]); distances_in [B,NC] is the vector of the state's
 * mask call (step 0's leg is distances_in[b, a_0], as in co_cvrptw_step); done, reward,
 * current_loc, distances and action_mask are written for the last step.  The final state is
 * that of the `steps` single calls bit for bit: a later step's leg distances[a] is
 * dist(locs[current_node], locs[a]), the same expression the single step's mask call
 * stored.  feasible (nullable, u8 [steps, B]): the value action_mask[b, a_t] had before
 * step t (0 for an a_t outside 0..N); time (nullable, f32 [steps, B]): current_time after
 * step t.  not_done counts the rows not done after the last step.  On the device a row's
 * coordinates, windows, durations, demands and visited set stay in registers for the whole
 * call; per step the action is read and feasible / time written. */
int co_cvrptw_steps(int64_t batch, int64_t num_loc, int64_t steps, const int64_t* actions,
                    int64_t act_stride_t, int64_t act_stride_b, const float* locs,
                    const float* demand, float* used, const float* vehicle_capacity,
                    uint8_t* visited, float* current_time, int64_t* current_node,
                    const float* distances_in, const void* durations, int dur_dtype,
                    const void* time_windows, int tw_dtype, uint8_t* done, uint8_t* reward,
                    float* current_loc, float* distances, uint8_t* action_mask,
                    uint8_t* feasible, float* time, int32_t* status, int32_t* not_done,
                    void* stream);

/* ---------------------------------------------------------------- MTVRP */

/* The multi-task VRP (rl4co/envs/routing/mtvrp/env.py): capacity plus any combination of
 * open routes (O), backhauls (B), a route-length limit (L) and time windows (TW), each row of
 * a batch its own variant.  N = customers, NC = N + 1 columns (the depot first), 1 <= N <=
 * CO_MTVRP_MAX_N, else CO_E_INVAL; an empty batch is a no-op; a NULL pointer not marked
 * nullable is CO_E_INVAL; locs and time_windows hold pairs and must be 8-byte aligned
 * (CO_E_ALIGN).
 *
 * Inputs, all f32 but the two byte arrays: locs [B, NC, 2]; time_windows [B, NC, 2] (start,
 * end; +inf end = no window); service_time, demand_linehaul, demand_backhaul [B, NC] (0 at the
 * depot); the per-row scalars vehicle_capacity, speed, distance_limit (+inf = no limit) [B, 1]
 * and open_route [B, 1] (u8, != 0 is open) -- taken from the td, not from the generator.
 * State: current_node [B] i64; current_time, current_route_length, used_capacity_linehaul,
 * used_capacity_backhaul [B, 1] f32; visited [B, NC] u8.
 *
 * Arithmetic.  Every operation is f32, each rounded on its own (no FMA, no fast-math,
 * correctly rounded sqrtf and /).  dist(p, q) is the CVRPTW section's sqrtf(dx*dx + dy*dy),
 * with the same one-ulp deviation from torch's norm.  A bool times a float is a
 * multiplication by 0.0f / 1.0f, so 0 * NaN and 0 * inf are NaN.  max is torch.max: NaN
 * when either operand is NaN.  Every compare is false for a NaN.
 *
 * The mask of a state (get_action_mask, env.py:212-279), with cur = clamp(current_node, 0,
 * N) for the coordinates, nopen = (float)!open_route, per column c = 0..N:
 *   d_ij[c]  = dist(locs[cur], locs[c])                                        :215-217
 *   d_j0[c]  = dist(locs[c], locs[0])                                          :218
 *   arr      = current_time + d_ij[c] / speed                                  :225
 *   reach    = arr < tw[c][1]                                                  :227
 *   depot_ok = ((max(arr, tw[c][0]) + service[c]) + d_j0[c] / speed) * nopen
 *              < tw[0][1]                                                      :230-232
 *   over     = (route_len + d_ij[c]) + d_j0[c] * nopen > distance_limit        :235-238
 *   lh_missing   = some unvisited column has demand_linehaul > 0               :242-244
 *   carrying_bh  = demand_backhaul[cur] > 0                                    :245-253
 *   demand_ok = (lh_missing && !(dl[c] + used_l > cap) && !carrying_bh && dl[c] > 0)
 *               || (!(db[c] + used_b > cap) && db[c] > 0)                      :254-266
 *   can[c]   = reach && depot_ok && demand_ok && !over && !visited[c]          :269-275
 *   can[0]   = !(current_node == 0 && any(can[1..N]))                          :278
 * The depot column ignores every other test.  lh_missing: the reference's sum(dl *
 * !visited) > 0 is exactly this for finite non-negative demands; a NaN, infinite or negative
 * linehaul demand makes the reference's sum differ (NaN: never missing), which is not
 * reproduced.
 *
 * The step (env.py:100-162), a = action[b]; an a outside 0..N sets CO_ST_INDEX_RANGE and
 * leaves the row's whole state (node, time, length, capacities, visited) as it was:
 *   leg = dist(locs[cur], locs[a])           -- recomputed, no stored distances vector
 *   current_time         = (float)(a != 0) * (max(current_time + leg / speed, tw[a][0])
 *                          + service[a])                                       :115-118
 *   current_route_length = (float)(a != 0) * (route_len + leg)                 :121-123
 *   used_l = (float)(a != 0) * (used_l + dl[a]); used_b likewise with db       :135-140
 *   visited[a] = 1; done = sum(visited) == NC; reward = 0.0f; current_node = a :143-147
 *   then the mask above on the new state.
 *
 * The reward (env.py:281-291): the legs depot -> a_0 -> ... -> a_{T-1} -> depot, a leg whose
 * destination is the depot counting 0 on an open row, summed in f64 in step order and
 * rounded once, negated (as co_cvrp_reward accumulates; 1e-5 relative to the reference, not
 * bit for bit).  An a outside 0..N sets CO_ST_INDEX_RANGE; its two legs are left out.
 *
 * Validity (check_solution_validity, env.py:294-365), one status bit per message, in the
 * reference's order; d0[c] = dist(locs[c], locs[0]):
 *   not (every customer exactly once, every other entry 0)      CO_ST_INVALID_TOUR     :301-306
 *   !(distance_limit >= 0)                                      CO_ST_MT_LIMIT_NEGATIVE   :309
 *   !(tw >= 0) (either end)                                     CO_ST_MT_TW_NEGATIVE      :313
 *   !(service >= 0)                                             CO_ST_MT_SERVICE_NEGATIVE :314
 *   !(tw[c][0] < tw[c][1])                                      CO_ST_MT_TW_INFEASIBLE :315-317
 *   !((tw[c][0] + d0[c]) + service[c] <= tw[0][1])              CO_ST_MT_DEPOT_RETURN  :318-321
 *       -- the bound is THIS ROW's depot deadline (the reference's indexing gives that here,
 *       unlike CVRPTW's batch row 0)
 *   the scan from the depot, len = t = 0, per action a (an a outside 0..N: CO_ST_INDEX_RANGE
 *   and CO_ST_INVALID_TOUR, no scan for the row), d = dist(locs[prev], locs[a]):
 *     len = len + d * (float)!(open && a == 0); !(len <= distance_limit)
 *                                                               CO_ST_MT_ROUTE_LIMIT   :333-338
 *     len = 0 when a == 0
 *     t = max(t + d, tw[a][0]); !(t <= tw[a][1])                CO_ST_MT_DEADLINE      :341-346
 *     t = t + service[a]; t = 0 when a == 0
 *       -- the scan adds d itself, not d / speed, and resets at the depot: as the reference
 *     ul = ul * (float)(a != 0) + dl[a]; !(ul <= cap)           CO_ST_MT_OVER_LINEHAUL :353-364
 *     ub likewise with db                                       CO_ST_MT_OVER_BACKHAUL
 *       -- against this row's vehicle_capacity (the reference broadcasts [B] against [B, 1]
 *       and so compares with every row's; equal when all capacities are, as generated) */
#define CO_MTVRP_MAX_N 1023

/* The instance inputs above, one pointer each, handed to every MTVRP entry but the reward
 * as one table in host memory; it is read during the call and need not outlive it.  A NULL
 * table or member is CO_E_INVAL (co_mtvrp_check does not read speed, which may be NULL). */
typedef struct co_mtvrp_instance {
  const float* locs;             /* [B, NC, 2], 8-byte aligned */
  const float* time_windows;     /* [B, NC, 2], 8-byte aligned */
  const float* service_time;     /* [B, NC] */
  const float* demand_linehaul;  /* [B, NC] */
  const float* demand_backhaul;  /* [B, NC] */
  const float* vehicle_capacity; /* [B, 1] */
  const float* speed;            /* [B, 1] */
  const float* distance_limit;   /* [B, 1] */
  const uint8_t* open_route;     /* [B, 1] */
} co_mtvrp_instance;

#define CO_ST_MT_LIMIT_NEGATIVE 2048     /* "Distance limits must be non-negative." */
#define CO_ST_MT_TW_NEGATIVE 4096        /* "Time windows must be non-negative." */
#define CO_ST_MT_SERVICE_NEGATIVE 8192   /* "Service time must be non-negative." */
#define CO_ST_MT_TW_INFEASIBLE 16384     /* "there are unfeasible time windows" */
#define CO_ST_MT_DEPOT_RETURN 32768      /* "vehicle cannot perform service and get back to
                                            depot in time." */
#define CO_ST_MT_ROUTE_LIMIT 65536       /* "Route exceeds distance limit" */
#define CO_ST_MT_DEADLINE 131072         /* "vehicle cannot start service before deadline" */
#define CO_ST_MT_OVER_LINEHAUL 262144    /* "Used more than capacity for demand_linehaul" */
#define CO_ST_MT_OVER_BACKHAUL 524288    /* "Used more than capacity for demand_backhaul" */

/* MTVRPEnv._reset (env.py:164-209) in one launch: the zeroed state at the depot and its
 * mask. */
int co_mtvrp_reset(int64_t batch, int64_t num_loc, const co_mtvrp_instance* instance,
                   int64_t* current_node, float* current_time, float* current_route_length,
                   float* used_linehaul, float* used_backhaul, uint8_t* visited,
                   uint8_t* action_mask, void* stream);

/* MTVRPEnv._step (env.py:100-162) in one launch: the update and the new mask.  Every output
 * is a buffer of its own, but visited_out may be visited_in.  status / not_done (nullable)
 * as in co_cvrptw_step.  One step moves 31 NC + 70 bytes per row (locs 8, windows 8,
 * service 4, two demands 8, visited 1 in and 1 out, the mask 1 per column; 70 of row
 * scalars) against 2 NC square roots and 2 NC divisions: bandwidth-bound. */
int co_mtvrp_step(int64_t batch, int64_t num_loc, const int64_t* action, const co_mtvrp_instance* instance,
                  const int64_t* current_in, const float* time_in, const float* route_length_in,
                  const float* used_linehaul_in, const float* used_backhaul_in,
                  const uint8_t* visited_in, int64_t* current_out, float* time_out,
                  float* route_length_out, float* used_linehaul_out, float* used_backhaul_out,
                  uint8_t* visited_out, uint8_t* done, float* reward, uint8_t* action_mask,
                  int32_t* status, int32_t* not_done, void* stream);

/* MTVRPEnv.get_action_mask alone (env.py:212-279). */
int co_mtvrp_action_mask(int64_t batch, int64_t num_loc, const co_mtvrp_instance* instance,
                         const int64_t* current_node, const float* current_time,
                         const float* current_route_length, const float* used_linehaul,
                         const float* used_backhaul, const uint8_t* visited,
                         uint8_t* action_mask, void* stream);

/* `steps` (>= 1) preset co_mtvrp_step calls in one launch: action (t, b) at
 * actions[t*act_stride_t + b*act_stride_b].  The state is updated in place; done, reward and
 * action_mask are written for the last step, the mask computed once, on the final state,
 * which is that of the `steps` single calls bit for bit.  Nullable per-step outputs, [steps,
 * B]: feasible (u8: the value action_mask[b, a_t] had before step t; 0 for an a_t outside
 * 0..N), time and route_length (f32: current_time / current_route_length after step t).
 * not_done counts the rows not done after the last step.  On the device the row stays in
 * registers for the whole call. */
int co_mtvrp_steps(int64_t batch, int64_t num_loc, int64_t steps, const int64_t* actions,
                   int64_t act_stride_t, int64_t act_stride_b, const co_mtvrp_instance* instance,
                   int64_t* current_node, float* current_time, float* current_route_length,
                   float* used_linehaul, float* used_backhaul, uint8_t* visited, uint8_t* done,
                   float* reward, uint8_t* action_mask, uint8_t* feasible, float* time,
                   float* route_length, int32_t* status, int32_t* not_done, void* stream);

/* MTVRPEnv._get_reward for actions [B, T] (element (b, t) at b*act_stride_b +
 * t*act_stride_t), as stated above; status nullable. */
int co_mtvrp_reward(int64_t batch, int64_t num_loc, int64_t steps, const float* locs,
                    const int64_t* actions, int64_t act_stride_b, int64_t act_stride_t,
                    const uint8_t* open_route, float* reward, int32_t* status, void* stream);

/* check_solution_validity for actions [B, T]: the status bits stated above. */
int co_mtvrp_check(int64_t batch, int64_t num_loc, int64_t steps,
                   const co_mtvrp_instance* instance, const int64_t* actions,
                   int64_t act_stride_b, int64_t act_stride_t, int32_t* status, void* stream);

/* ------------------------------------------------------------------ PDP */

/* The pickup-and-delivery problem (rl4co/envs/routing/pdp/env.py:20-234).  N = num_loc
 * (even), h = N / 2, NC = N + 1 columns: column 0 is the depot, 1..h the pickups, h+1..N the
 * deliveries; pickup p pairs with delivery p + h.  2 <= N <= CO_PDP_MAX_N and N even, else
 * CO_E_INVAL from every entry, decided before the empty-batch return (an empty batch is a
 * no-op); a NULL pointer not marked nullable is CO_E_INVAL.  available, to_deliver and
 * action_mask are byte rows [B, NC]; a non-zero input byte counts as 1 and every output
 * byte is 0 or 1.
 *
 * Reset (env.py:108-151):
 *   locs[b]       = cat(depot[b], locs_in[b])            [NC, 2]
 *   to_deliver[c] = c <= h        (h + 1 ones, then h zeros)
 *   available[c]  = 1
 *   action_mask[c] = c == 0       -- NOT available & to_deliver: the first step is the depot
 *   current_node = i = 0 [B,1]; done = terminated = 0 [B,1]
 *
 * Step (env.py:67-106), a = action[b]:
 *   pair = (a + h) % NC           (a pickup's delivery; the depot's pair is column h and a
 *                                  delivery's a column 0..h-1, which reset left at 1 -- the
 *                                  reference applies the rule to every action, so do we)
 *   available[a] = 0 ; to_deliver[pair] = 1
 *   action_mask  = available & to_deliver   -- from the two rows, never from the old mask
 *   done = no column of available left ; reward = 0 (bool) ; i + 1 ; current_node = a
 * An a outside 0..N sets CO_ST_INDEX_RANGE (torch's scatter raises) and edits neither row;
 * i, current_node, done and the mask are written all the same.
 *
 * Reward (env.py:189-199) for actions [B, T]: minus the closed length of the tour
 * [locs[0], locs[a_0], ..., locs[a_{T-1}]] over locs[b % locs_batch]: the T + 1 legs
 * dist(p, q) = sqrtf(dx*dx + dy*dy) in f32 (every operation rounded on its own, as
 * co_tsp_reward's), added in tour order in f64 from 0, the closing leg to the depot last,
 * and rounded once: reward = -(float)sum.  A rollout from the depot has a zero first leg;
 * one that starts at a pickup (multistart) visits the depot twice.  An a outside 0..N sets
 * CO_ST_INDEX_RANGE and the legs that touch it are left out.
 *
 * Validity (env.py:201-216), check != 0, T odd (an even T with check is CO_E_INVAL: the
 * reference's two slices then differ in length), T2 = T / 2, per row:
 *   sort(actions) != arange(T): some value outside 0..T-1 or twice   CO_ST_PDP_NOT_ALL_NODES
 *   else, pos = argsort(actions): !(pos[k] < pos[T2 + k]) for a k in 1..T2
 *                                                                     CO_ST_PDP_PRECEDENCE
 * On a permutation pos[k] < pos[T2 + k] says that value T2 + k appears after value k, which
 * is tested when T2 + k is met in tour order.  A row that is not a permutation sets the
 * first bit only (the reference's first assert ends the check). */
#define CO_PDP_MAX_N 2046
#define CO_ST_PDP_NOT_ALL_NODES 1048576  /* "Not visiting all nodes"       pdp/env.py:203-208 */
#define CO_ST_PDP_PRECEDENCE 2097152     /* "Deliverying without pick-up"  pdp/env.py:210-216 */

/* PDPEnv._reset (env.py:108-151) in one launch: every tensor stated above; depot [B,2],
 * locs_in [B,N,2], locs_out [B,NC,2] (pairs: 8-byte aligned, else CO_E_ALIGN). */
int co_pdp_reset(int64_t batch, int64_t num_loc, const float* depot, const float* locs_in,
                 float* locs_out, uint8_t* available, uint8_t* to_deliver, uint8_t* action_mask,
                 int64_t* current_node, int64_t* i, uint8_t* done, uint8_t* terminated,
                 void* stream);

/* PDPEnv._step (env.py:67-106) in one launch, out of place (the reference's scatter is):
 * every output is a buffer of its own, though available_out / to_deliver_out may be their
 * inputs (a lane reads the columns it writes).  i [B,1], current_out [B,1], done / reward
 * [B].  One step moves 5 NC + 34 bytes per row (two byte rows in, three out; the action, i
 * in and out, current_node, done and reward): 539 B at N = 100. */
int co_pdp_step(int64_t batch, int64_t num_loc, const int64_t* action,
                const uint8_t* available_in, const uint8_t* to_deliver_in,
                uint8_t* available_out, uint8_t* to_deliver_out, uint8_t* action_mask,
                const int64_t* i_in, int64_t* i_out, int64_t* current_out, uint8_t* done,
                uint8_t* reward, int32_t* status, void* stream);

/* `steps` (>= 1) preset co_pdp_step calls in one launch: action (t, b) at
 * actions[t*act_stride_t + b*act_stride_b].  available / to_deliver / i / current_node are
 * updated in place; action_mask (a buffer of its own), done and reward are written for the
 * last step.  The final state is that of the `steps` single calls bit for bit.  feasible
 * (nullable, u8 [steps, B]): the value action_mask[b, a_t] had before step t -- step 0 reads
 * mask_in[b, a_0] (the caller's mask: after a reset it is not available & to_deliver), a
 * later step tests available & to_deliver -- and 0 for an a_t outside 0..N.  On the device a
 * row's two sets are bit words in registers for the whole call (32 columns per lane); per
 * step the action is read and feasible written, the byte rows are stored once: 9 bytes
 * per row-step plus 5 NC + 27 per row. */
int co_pdp_steps(int64_t batch, int64_t num_loc, int64_t steps, const int64_t* actions,
                 int64_t act_stride_t, int64_t act_stride_b, const uint8_t* mask_in,
                 uint8_t* available, uint8_t* to_deliver, uint8_t* action_mask, int64_t* i,
                 int64_t* current_node, uint8_t* done, uint8_t* reward, uint8_t* feasible,
                 int32_t* status, void* stream);

/* PDPEnv.get_reward for actions [B, T] (element (b, t) at b*act_stride_b + t*act_stride_t,
 * 1 <= T <= 2048) on locs [locs_batch, NC, 2] (batch % locs_batch == 0; 8-byte aligned), and
 * with check != 0 the two validity bits, in one pass over the row, as stated above. */
int co_pdp_reward(int64_t batch, int64_t num_loc, int64_t steps, const float* locs,
                  int64_t locs_batch, const int64_t* actions, int64_t act_stride_b,
                  int64_t act_stride_t, int check, float* reward, int32_t* status,
                  void* stream);

/* co_decode_step fused with co_pdp_step for the selected action (the evaluated one in
 * CO_DECODE_EVALUATE), device build only: logits [B, NC] (row stride logits_stride) and
 * action_mask (the decode's mask) are read once, with available_in / to_deliver_in; the
 * outputs are co_decode_step's (action_out, logp_sel, the status bits) and co_pdp_step's
 * (available_out, to_deliver_out, mask_out = available & to_deliver, i_out, current_out,
 * done, step_reward), the same bits as the two calls.  ll_accum (nullable) += logp_sel, as
 * in co_tsp_decode_step.  mode: CO_DECODE_GREEDY / SAMPLING / EVALUATE with the FAST /
 * CERTIFIED flags.  NC is odd, so the rows run on the byte-wise row engines.  mask_out may
 * be action_mask (the mask edited in place): that call runs as the two launches and, like
 * every two-launch route, refuses ll_accum (CO_E_INVAL).  A row-step
 * reads 7 NC + 8 bytes (logits 4 NC, three byte rows, i) and writes 3 NC + 30 (three byte
 * rows; action, logp, i, current_node, done, reward): 1,048 B at N = 100. */
int co_pdp_decode_step(int64_t batch, int64_t num_loc, const float* logits,
                       int64_t logits_stride, const uint8_t* action_mask, float tanh_clipping,
                       float temperature, int mode, const int64_t* action_in,
                       int64_t* action_out, float* logp_sel, uint64_t seed, uint64_t offset,
                       const uint8_t* available_in, const uint8_t* to_deliver_in,
                       uint8_t* available_out, uint8_t* to_deliver_out, uint8_t* mask_out,
                       const int64_t* i_in, int64_t* i_out, int64_t* current_out, uint8_t* done,
                       uint8_t* step_reward, float* ll_accum, int32_t* status, void* stream);

/* ------------------------------------------------------------------- OP */

/* The orienteering problem (rl4co/envs/routing/op/env.py:24-262, Kool et al.'s OP): collect
 * prizes on a tour from and back to the depot whose length stays below max_length.  N =
 * num_loc, NC = N + 1 columns, column 0 the depot.  1 <= N <= CO_OP_MAX_N, else CO_E_INVAL
 * from every entry, decided before the empty-batch return (an empty batch is a no-op); a NULL
 * pointer not marked nullable is CO_E_INVAL; locs hold pairs and must be 8-byte aligned
 * (CO_E_ALIGN).  visited and action_mask are byte rows [B, NC]; a non-zero input byte counts
 * as 1 and every output byte is 0 or 1.  CO_OP_MAX_N is bounded by the fused decode step,
 * which keeps a lane's columns of locs and max_length in registers beside its logits: 16
 * columns a lane on the 1,024-column row engine, the widest that does so without scratch.
 *
 * dist(p, q) is the CVRPTW section's sqrtf(dx*dx + dy*dy) in f32, every operation rounded on
 * its own (no FMA); it is symmetric bit for bit.
 *
 * Reset (env.py:110-151):
 *   locs[b]          = cat(depot[b], locs_in[b])                      [NC, 2]
 *   prize[b]         = cat(0, prize_in[b])                            [NC]
 *   max_length[b, c] = (max_length_in[b] - dist(depot[b], locs[b, c])) - 1e-6f   [NC], in
 *                      f32, in that order: the length allowed on ARRIVAL at c
 *   tour_length = current_total_prize = 0 [B] (f32); current_node = 0 [B,1]; i = 0 [B]
 *   visited = 0 [B, NC], and the mask below on that state
 *
 * The mask (get_action_mask, env.py:153-169) of a state (visited, tour_length,
 * current_node), c = 0..N:
 *   cur        = locs[b, clamp(current_node, 0, N)]
 *   exceeds[c] = tour_length + dist(locs[b, c], cur) > max_length[b, c]
 *                -- one f32 add and one f32 compare, false for a NaN: a column with a NaN
 *                coordinate (or a NaN tour_length) is never closed by the length test
 *   mask[c]    = !(visited[c] | visited[0] | exceeds[c]);  mask[0] = 1 always
 *
 * The step (env.py:74-108), a = action[b]:
 *   tour_length        += dist(locs[a], locs[clamp(current_node_in, 0, N)])
 *   current_total_prize += prize[a]                                    (f32)
 *   visited[a] = 1;  done = (a == 0) & (i_in > 0);  i + 1;  current_node = a
 *   reward = 0 (bool, zeros_like(done)); then the mask above on the new state
 * Two consequences of the reference's rule are kept:
 *   - action 0 at i == 0 sets visited[0], so every customer closes; it does not set done;
 *   - a row that is done goes on taking action 0 (the rollout pads with it): visited[0]
 *     stays set, the leg is 0, and done stays 1.
 * An a outside 0..N sets CO_ST_INDEX_RANGE (torch's scatter raises) and leaves visited,
 * tour_length and current_total_prize unchanged; i + 1, current_node = a (so the next mask
 * and leg take locs[clamp(a, 0, N)]), done by the rule above and the mask are written all
 * the same -- the rule co_cvrptw_step and co_pdp_step state.
 *
 * Reward (env.py:171-180) for actions [B, T]: the sum of prize[b % prize_batch, a_t], added
 * in tour order in f64 from 0 and rounded once.  An a_t outside 0..N sets CO_ST_INDEX_RANGE
 * and adds nothing.  With T = 1 the reward is 0 and a non-zero action sets
 * CO_ST_OP_SINGLE_NONZERO (the reference's assert).
 *
 * Validity (env.py:182-214), check != 0, per row:
 *   a customer (1..N) met twice                                       CO_ST_OP_DUPLICATE
 *   else len = the closed tour length of locs[a_0], ..., locs[a_{T-1}]: the T legs
 *   dist(locs[a_t], locs[a_{t+1}]), the last one back to a_0, each in f32, added in tour
 *   order in f64 from 0 and rounded once to f32 (legs that touch an a_t outside 0..N are
 *   left out);
 *   !(len <= (max_length[c] + dist(locs[0], locs[c]) + 1e-6f) + 1e-5f) for a column c, in
 *   f32, left to right                                                CO_ST_OP_LENGTH
 * A duplicate row sets the first bit alone (the reference's first assert ends the check). */
#define CO_OP_MAX_N 1023
#define CO_ST_OP_DUPLICATE 4194304        /* "Duplicates"                      op/env.py:194-197 */
#define CO_ST_OP_LENGTH 8388608           /* "Max length exceeded by ..."      op/env.py:210-214 */
#define CO_ST_OP_SINGLE_NONZERO 16777216  /* "If all length 1 tours, they should be zero" :175 */

/* OPEnv._reset (env.py:110-151) in one launch: every tensor stated above.  depot [B,2],
 * locs_in [B,N,2], prize_in [B,N], max_length_in [B]; locs_out [B,NC,2], prize_out and
 * max_length_out [B,NC].  A row moves 12 N + 12 bytes in and 18 NC + 24 out. */
int co_op_reset(int64_t batch, int64_t num_loc, const float* depot, const float* locs_in,
                const float* prize_in, const float* max_length_in, float* locs_out,
                float* prize_out, float* max_length_out, float* tour_length,
                float* current_total_prize, int64_t* current_node, int64_t* i,
                uint8_t* visited, uint8_t* action_mask, void* stream);

/* OPEnv._step (env.py:74-108) in one launch, out of place: every output is a buffer of its
 * own, though visited_out may be visited_in (a lane reads the columns it writes).  locs,
 * prize and max_length are the post-reset [B,NC,..]; tour_length / current_total_prize / i
 * / done / reward [B], current_node [B,1].  One step reads 13 NC + 52 bytes per row (locs 8
 * NC, max_length 4 NC, visited NC; the action, two gathered locs, a prize, four scalars) and
 * writes 2 NC + 26 (visited, the mask, five scalars, done, reward): 1,593 B at N = 100,
 * against NC square roots. */
int co_op_step(int64_t batch, int64_t num_loc, const int64_t* action, const float* locs,
               const float* prize, const float* max_length, const uint8_t* visited_in,
               uint8_t* visited_out, const float* tour_length_in, float* tour_length_out,
               const float* total_prize_in, float* total_prize_out,
               const int64_t* current_in, int64_t* current_out, const int64_t* i_in,
               int64_t* i_out, uint8_t* done, uint8_t* reward, uint8_t* action_mask,
               int32_t* status, void* stream);

/* OPEnv.get_action_mask alone (env.py:153-169): 13 NC + 20 bytes read, NC written a row. */
int co_op_action_mask(int64_t batch, int64_t num_loc, const float* locs,
                      const float* max_length, const uint8_t* visited,
                      const float* tour_length, const int64_t* current_node,
                      uint8_t* action_mask, void* stream);

/* `steps` (>= 1) preset co_op_step calls in one launch: action (t, b) at
 * actions[t*act_stride_t + b*act_stride_b].  visited / tour_length / current_total_prize /
 * current_node / i are updated in place; action_mask (a buffer of its own), done and reward
 * are those of the last step.  The final state is that of the `steps` single calls bit for
 * bit.  feasible (nullable, u8 [steps, B]): the value action_mask[b, a_t] had before step t
 * -- step 0 reads mask_in[b, a_0] (the caller's mask), a later step evaluates the mask rule
 * for column a_t alone -- and 0 for an a_t outside 0..N.  length (nullable, f32 [steps, B]):
 * tour_length after step t.  On the device a row's visited set is bit words in registers
 * for the whole call and the row scalars live on every lane of the row's group; a step
 * reads the action, locs[a] and prize[a] (and max_length[a] for feasible): 20 bytes a
 * row-step, 5 more written with feasible and length, plus 15 NC + 58 once per row. */
int co_op_steps(int64_t batch, int64_t num_loc, int64_t steps, const int64_t* actions,
                int64_t act_stride_t, int64_t act_stride_b, const float* locs,
                const float* prize, const float* max_length, const uint8_t* mask_in,
                uint8_t* visited, float* tour_length, float* current_total_prize,
                int64_t* current_node, int64_t* i, uint8_t* done, uint8_t* reward,
                uint8_t* action_mask, uint8_t* feasible, float* length, int32_t* status,
                void* stream);

/* OPEnv.get_reward for actions [B, T] (element (b, t) at b*act_stride_b + t*act_stride_t,
 * 1 <= T <= 2^20) on prize [prize_batch, NC] (batch % prize_batch == 0) and, with check !=
 * 0, the validity bits on locs [locs_batch, NC, 2] and max_length [locs_batch, NC] (batch %
 * locs_batch == 0; both may be NULL without check), in one pass over the row, as stated
 * above: 12 bytes a tour step (20 with check) and 16 NC a row for the length test. */
int co_op_reward(int64_t batch, int64_t num_loc, int64_t steps, const float* prize,
                 int64_t prize_batch, const float* locs, const float* max_length,
                 int64_t locs_batch, const int64_t* actions, int64_t act_stride_b,
                 int64_t act_stride_t, int check, float* reward, int32_t* status,
                 void* stream);

/* The post-reset instance tensors of OP, one pointer each, handed to co_op_decode_step as one
 * table in host memory (the entry's arguments stay within the 28 integer-class slots every
 * entry of this header keeps to); it is read during the call and need not outlive it.  A
 * NULL table or member is CO_E_INVAL. */
typedef struct co_op_instance {
  const float* locs;       /* [B, NC, 2], 8-byte aligned */
  const float* prize;      /* [B, NC] */
  const float* max_length; /* [B, NC] */
} co_op_instance;

/* co_decode_step fused with co_op_step for the selected action (the evaluated one in
 * CO_DECODE_EVALUATE), device build only: logits [B, NC] (row stride logits_stride) and
 * action_mask (the decode's mask) are read once, with the row's visited, locs and
 * max_length; the outputs are co_decode_step's (action_out, logp_sel, the status bits) and
 * co_op_step's, the same bits as the two calls.  ll_accum (nullable) += logp_sel, as in
 * co_tsp_decode_step.  mode: CO_DECODE_GREEDY / SAMPLING / EVALUATE with the FAST /
 * CERTIFIED flags.  Every output is a buffer of its own; mask_out may be action_mask (the
 * mask edited in place): that call runs as the two launches and, like every two-launch
 * route, refuses ll_accum (CO_E_INVAL).  A row-step reads 18 NC + 44 bytes (logits 4 NC, two
 * byte rows, locs 8 NC, max_length 4 NC, the scalars and gathers of co_op_step less the
 * action) and writes 2 NC + 38: 2,102 B at N = 100, against 2,110 B for the two calls -- the fused step
 * saves a launch, not traffic. */
int co_op_decode_step(int64_t batch, int64_t num_loc, const float* logits,
                      int64_t logits_stride, const uint8_t* action_mask, float tanh_clipping,
                      float temperature, int mode, const int64_t* action_in,
                      int64_t* action_out, float* logp_sel, uint64_t seed, uint64_t offset,
                      const co_op_instance* instance, const uint8_t* visited_in,
                      uint8_t* visited_out, const float* tour_length_in, float* tour_length_out,
                      const float* total_prize_in, float* total_prize_out,
                      const int64_t* current_in, int64_t* current_out, const int64_t* i_in,
                      int64_t* i_out, uint8_t* done, uint8_t* step_reward, uint8_t* mask_out,
                      float* ll_accum, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* CO_ENV_H */
