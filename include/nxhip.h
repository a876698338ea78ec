/*
 * nxhip.h -- C ABI of the MI355X-native assemble + solve path for the hydraulic
 * network saddle-point system of networks_fenicsx.
 *
 * The reference has no C/FFI boundary of its own: its hot path sits behind the
 * Python classes HydraulicNetworkAssembler and Solver, which hand petsc4py
 * Mat/Vec/KSP objects to DOLFINx C++ and PETSc/MUMPS. Each entry point below
 * names the reference interface it replaces (file:line under
 * /root/reference/src/networks_fenicsx/). The Python binding is
 * networks_fenicsx_amd/_lib.py (ctypes); INTEGRATION.md shows the stub a
 * maintainer would add on the reference side.
 *
 * Conventions
 *   - every function returns NX_OK (0) or a negative NX_ERR_* code; the message
 *     of the last failure on the calling thread is nx_last_error();
 *   - host arrays are caller-owned and copied in/out; device buffers are owned by
 *     the opaque handle and released by nx_destroy;
 *   - calls on one handle must be serialised by the caller (the Python layer holds
 *     the GIL); all work is issued on the handle's own HIP stream.
 *
 * Device layout (per rank): every local graph edge owns 2N+1 consecutive DoFs,
 * interleaved [q_0, p_0, q_1, p_1, ..., p_{N-1}, q_N] (P1 flux vertices and DG0
 * pressure cells, source -> target), then one multiplier per owned bifurcation.
 * Columns >= n_own are ghosts (multipliers or flux end values owned by another
 * rank). The pressure rows are negated so the assembled matrix is symmetric
 * (the solution is unchanged); MINRES requires symmetry.
 */
#ifndef NXHIP_H
#define NXHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NX_OK 0
#define NX_ERR_ARG -1     /* invalid argument / shape */
#define NX_ERR_HIP -2     /* HIP runtime failure */
#define NX_ERR_RCCL -3    /* RCCL failure */
#define NX_ERR_STATE -4   /* call out of order (e.g. solve before assemble) */
#define NX_ERR_NOCONV -5  /* MINRES did not reach the tolerance in maxit */

#define NX_UNIQUE_ID_BYTES 128

typedef struct nx_network nx_network_t;
typedef struct nx_group nx_group_t;

/* Library/ABI version (major*10000 + minor*100 + patch). */
int nx_version(void);

/* Message of the last failure on this thread ("" if none). */
const char* nx_last_error(void);

/* Number of visible HIP devices. */
int nx_device_count(int32_t* count);

/*
 * Create a network handle on `device` and build the CSR sparsity pattern on it.
 * Replaces Solver.__init__'s fem.petsc.create_matrix / create_vector
 * (solver.py:43-49) and the DoF layout of HydraulicNetworkAssembler.__init__
 * (assembly.py:121-162).
 *
 *   N          cells per edge (>= 1)
 *   n_edges    local edges E
 *   edge_x     E*6 doubles: source xyz, target xyz (gdim < 3 padded with 0)
 *   edge_lm    E*2 int32: column of the multiplier at the source / target end,
 *              -1 when that end is not a bifurcation
 *   n_lm       owned multiplier rows B
 *   lm_rowptr  B+1 int32 CSR offsets of the multiplier rows
 *   lm_col     int32 columns (sorted ascending per row): flux end DoFs
 *   lm_val     double values (+1 at an in-edge end q_N, -1 at an out-edge start q_0;
 *              assembly.py:271-277)
 *   n_ghost    ghost columns appended after the n_own = E*(2N+1)+B owned ones
 */
int nx_create(int32_t device, int32_t N, int64_t n_edges, const double* edge_x,
              const int32_t* edge_lm, int64_t n_lm, const int32_t* lm_rowptr,
              const int32_t* lm_col, const double* lm_val, int64_t n_ghost,
              nx_network_t** out);

/*
 * General element degrees: HydraulicNetworkAssembler(mesh, flux_degree=k,
 * pressure_degree=m) (assembly.py:121-146) -- P_k equispaced flux per edge, DG0 (m = 0)
 * or continuous P_m pressure. No tree preconditioner (plain MINRES). The host
 * (networks_fenicsx_amd/layout_fe.py) numbers the DoFs, gives the sorted CSR pattern and
 * lists, for every nonzero and every rhs row, its terms in summation order; the device
 * evaluates them on every nx_assemble (k_assemble_fe: one thread per nonzero / row):
 *
 *   term (idx, ent) = table_val[ent] x factor, factor by table_kind[ent]:
 *     0 constant 1 | 1 R_e h_c (mass; idx = cell e*N + c) | 2 f h_c (source; idx = cell)
 *     | 3 edge_bc[idx] (boundary rhs; idx = 2e + end)
 *   h_c is the cell length from edge_x, computed like the reference mesh generator.
 *
 *   n_rows, rowptr (n_rows+1), col   the symmetric system's CSR pattern (sorted rows)
 *   n_ghost                          several ranks: columns n_rows.. are ghosts
 *                                    (layout_fe.build_fe_rank_layout / build_fe_partition;
 *                                    nx_comm_init then gives the halo plan, as for
 *                                    nx_create); 0 on one rank. n_edges may then count
 *                                    ghost edges too (coefficients, no rows)
 *   n_table, table_kind, table_val   the term table (reference element tensors, signs)
 *   a_ptr (nnz+1), a_idx, a_ent      the terms of every nonzero
 *   b_ptr (n_rows+1), b_idx, b_ent   the terms of every rhs row
 * nx_set_coefficients, nx_assemble, nx_solve and the getters work as for nx_create.
 */
int nx_create_fe(int32_t device, int32_t N, int64_t n_edges, const double* edge_x,
                 int64_t n_rows, const int32_t* rowptr, const int32_t* col, int64_t n_ghost,
                 int32_t n_table, const int32_t* table_kind, const double* table_val, const int32_t* a_ptr,
                 const int32_t* a_idx, const int32_t* a_ent, const int32_t* b_ptr,
                 const int32_t* b_idx, const int32_t* b_ent, nx_network_t** out);

/*
 * The flux degree k when nx_create_fe's tables are exactly a (k, 0) layout's
 * (layout_fe.build_fe_layout with m = 0: every entry's and every rhs row's term list equals
 * the closed form fe_s_terms gives without the tables), else 0. Exported so the host (and
 * the CPU tests) can probe the closed form without a device. Replaces nothing in the
 * reference: its forms are compiled per degree by FFCx (assembly.py:121-146).
 */
int nx_fe_struct_degree(int32_t N, int64_t n_edges, int64_t n_rows, const int32_t* rowptr,
                        const int32_t* col, int32_t n_table, const int32_t* a_ptr,
                        const int32_t* a_idx, const int32_t* a_ent, const int32_t* b_ptr,
                        const int32_t* b_idx, const int32_t* b_ent, int32_t* k_out);

/*
 * The edge templates of a general-degree handle (nx_create_fe builds them when every edge's
 * rows match one of a few shapes): *n_shapes = their number, 0 when the handle kept the
 * gather tables; *rows_per_edge = the rows of one edge. The assembly (k_fe_tasm) and the
 * direct solves' true residual (k_fe_tres) then read no gather tables and no CSR.
 */
int nx_fe_templates(nx_network_t* h, int32_t* n_shapes, int32_t* rows_per_edge);

/* Release every device buffer, graph and communicator of the handle. */
int nx_destroy(nx_network_t* h);

/* Local sizes: owned rows, columns (owned + ghosts), nonzeros. */
int nx_dims(nx_network_t* h, int64_t* n_rows, int64_t* n_cols, int64_t* nnz);

/*
 * Coefficients of the forms (HydraulicNetworkAssembler.compute_forms,
 * assembly.py:165-262), uploaded once and kept resident in HBM:
 *   edge_R   E doubles (per-edge resistance) or NULL to use R_const everywhere
 *   f        constant source term of the pressure equation
 *   edge_bc  E*2 doubles: rhs contribution at q_0 and q_N of each edge
 *            (-p_bc(source) at an inlet root, +p_bc(target) at an outlet leaf,
 *            0 elsewhere; assembly.py:258-260)
 * edge_R NULL with R_const NaN keeps the resident R (NX_ERR_STATE if none was ever set): only
 * f and edge_bc change, R is not uploaded and the matrix's version does not move -- what a
 * loop over scenarios uses between two right-hand-side assemblies.
 */
int nx_set_coefficients(nx_network_t* h, const double* edge_R, double R_const, double f,
                        const double* edge_bc);

/*
 * Spatially varying source of the mass-conservation equation (the `f` of compute_forms,
 * assembly.py:201-202, 262, given as one value per local edge): edge_f[E] replaces the
 * constant f of nx_set_coefficients in the pressure rhs (f_e h per cell, times the pressure
 * basis integrals for general degrees); NULL returns to the constant.
 */
int nx_set_source(nx_network_t* h, const double* edge_f);

/*
 * Assemble matrix values and/or rhs on the device into the resident CSR.
 * Replaces HydraulicNetworkAssembler.assemble (assembly.py:329-368) and
 * Solver.assemble (solver.py:90-101). Asynchronous on the handle's stream.
 */
int nx_assemble(nx_network_t* h, int32_t lhs, int32_t rhs);

/*
 * Solve on the device; replaces the KSP solve of Solver.solve (solver.py:107-135; default
 * there: preonly + LU/MUMPS). MINRES (Paige-Saunders) by default, or the direct tree solve
 * where nx_set_solver asked for it and it is exact (then iters = 1, or 2 after one
 * refinement step, and relres is the true residual ||b - A x|| / ||b||).
 *   rtol         stop when the MINRES residual estimate ||r_k|| / ||b|| <= rtol
 *   maxit        iteration cap
 *   check_every  iterations per host convergence check (graph chunk), >= 2, even
 *   iters/relres/converged  outputs (host)
 * Returns NX_OK also when not converged; `converged` tells. The solution stays on
 * the device (nx_get_solution copies it out).
 */
int nx_solve(nx_network_t* h, double rtol, int32_t maxit, int32_t check_every,
             int32_t* iters, double* relres, int32_t* converged);

/*
 * Tree Schur-complement preconditioner for MINRES: by default the exact one,
 * P = blockdiag(M, G^T M^{-1} G) with M the consistent flux mass (3 iterations), or with the
 * lumped mass D (nx_set_pc_exact; networks_fenicsx_amd/precond.py derives both and builds
 * these arrays). There is no reference counterpart: the reference factorises with MUMPS
 * (solver.py:58-65); this makes the iterative replacement converge in 3 iterations.
 * enable = 0 switches back to unpreconditioned MINRES. Chains (one per local edge, in job
 * order): edge slot, flip (chain runs target -> source), top / bottom junction slot (-1 =
 * ground). Junction slots (one per owned multiplier, level order per job): multiplier row,
 * chain to the parent, parent slot, CSR of chains hanging below (dc_lo: bottom slot of each
 * entry, slot_plam: the parent's multiplier row -- both derivable, passed to save the
 * kernels a dependent load). Jobs (one workgroup each):
 * chain ranges and level ranges; lvl_slot_off / top_lvl_off: slot offsets per level (root
 * level first) of the lower jobs / of the single top workgroup. Requires N <= 1024.
 * With several ranks the slots also cover the ghost junctions at the ends of local edges
 * (slot_lam = their ghost column) and nx_set_coarse must follow.
 */
int nx_set_preconditioner(nx_network_t* h, int32_t enable, int64_t n_chains,
                          const int32_t* chain_edge, const int32_t* chain_flip,
                          const int32_t* chain_up, const int32_t* chain_lo, int64_t n_slots,
                          const int32_t* slot_lam, const int32_t* slot_pchain,
                          const int32_t* slot_parent, const int32_t* slot_dc_off,
                          const int32_t* slot_dc, const int32_t* dc_lo, const int32_t* slot_plam,
                          int32_t n_jobs, const int32_t* job_chain_off,
                          const int32_t* job_lvl_off, int32_t n_lvl, const int32_t* lvl_slot_off,
                          int32_t n_top_lvl, const int32_t* top_lvl_off);

/*
 * Dense top part (single rank): the down kernel computes the top junction values it
 * needs as rows of G (inverse of the top tree Schur matrix, built once per solve) times
 * the top inputs, which removes the one-workgroup top kernel from every iteration.
 *   job_tslot_off/job_tslot  top slots each job updates and writes (round-robin)
 *   job_need_off/job_need    top slots whose values each job reads (<= 64 per job)
 *   top_uoff[n_top+1]        the top inputs a_s = sum of u[top_uoff[s] .. top_uoff[s+1]),
 *                            posted by the up kernel at fixed places: slot_uy (y' of a top
 *                            slot), chain_uit / chain_uib (I_top / I_bot of a chain, -1 =
 *                            none), job_root_u (kappa J_root + I_top of the root's parent
 *                            chain, kappa = dc entry job_root_dc) -- precond.py
 * Ignored (kept off) with several ranks or when the LDS kernels are not in use;
 * NXHIP_PC_DENSE=0 disables it. Call after nx_set_preconditioner.
 */
int nx_set_pc_dense(nx_network_t* h, int32_t enable, int32_t n_jobs, const int32_t* job_tslot_off,
                    const int32_t* job_tslot, const int32_t* job_need_off,
                    const int32_t* job_need, const int32_t* top_uoff, const int32_t* slot_uy,
                    const int32_t* chain_uit, const int32_t* chain_uib,
                    const int32_t* job_root_u, const int32_t* job_root_dc);

/*
 * Flux mass of the preconditioner: 1 (default) = the consistent P1 mass M, i.e. the exact
 * Schur complement P = blockdiag(M, G^T M^{-1} G) -- P^{-1} A has three distinct eigenvalues
 * and MINRES converges in 3 iterations; 0 = the lumped mass D (O(30) iterations). The
 * junction elimination is the same for both (precond.py, "Exact variant"); only the chain
 * outputs differ. NXHIP_PC_EXACT=0 makes 0 the default. Call after nx_set_preconditioner.
 */
int nx_set_pc_exact(nx_network_t* h, int32_t enable);
int nx_get_pc_exact(nx_network_t* h, int32_t* enabled);

/*
 * Sweep kernels of the preconditioner / direct solve: nx_get_pc_kernels reports whether the
 * uploaded decomposition runs the LDS kernels (1) or the global-memory ones (0, a job over
 * the LDS caps); nx_set_pc_kernels(h, 1) makes the next nx_set_preconditioner take the
 * global-memory kernels even where LDS fits. Several ranks must agree (their exchange
 * schedules differ): the host reduces the ranks' choice (MIN) and re-uploads -- the
 * reference's MPI-collective setup of the solver (solver.py:32-73) in one flag.
 */
int nx_set_pc_kernels(nx_network_t* h, int32_t global);
int nx_get_pc_kernels(nx_network_t* h, int32_t* lds);
/*
 * The lane shapes of the uploaded preconditioner (read only; tests pin the selection with
 * it): a chain is run by W lanes of CPL cells each. sweep_*: the shape of the sweep kernels.
 * step_*: the shape the one-launch / exchange step has for the handle's N, or (0, 0) where no
 * one-launch instantiation exists (N > 256). NX_ERR_STATE without a preconditioner.
 */
int nx_get_lane_shapes(nx_network_t* h, int32_t* sweep_w, int32_t* sweep_cpl, int32_t* step_w,
                       int32_t* step_cpl);

/*
 * Which solve nx_solve runs. solver = 0 (default): MINRES. solver = 1: the direct solve
 * the reference's default options ask for (ksp_type=preonly + pc_type=lu + MUMPS,
 * solver.py:58-65), specialised to the network: a block LU of [[M, K], [K^T, 0]] whose
 * Schur complement K^T M^{-1} K is inverted by the tree preconditioner's sweeps --
 *   y = M^{-1} b_q,  x_s = S^{-1} (K^T y - b_s),  x_q = M^{-1} (b_q - K x_s)
 * -- one HIP graph, followed by the true residual ||b - A x|| / ||b|| (one CSR SpMV),
 * which is what nx_solve reports (iters = 1). It runs when it is exact: one rank, the
 * consistent-mass preconditioner (nx_set_pc_exact 1) and tree_exact != 0 (the host
 * decomposition grounded no cycle-closing chain; precond.py TreePreconditioner.tree_exact).
 * Otherwise, or if the residual misses rtol, nx_solve runs MINRES. nx_get_solver returns
 * the requested solver and what the last nx_solve ran (0 MINRES, 1 direct).
 */
int nx_set_solver(nx_network_t* h, int32_t solver, int32_t tree_exact);
int nx_get_solver(nx_network_t* h, int32_t* requested, int32_t* last_run);
/*
 * Graphs with cycles (one rank): the direct solve stays exact, as MUMPS' LU is on any graph
 * (solver.py:58-65; the reference's own cyclic graph, tests/test_edge_info.py:8-35). The
 * decomposition grounds one end of each of the n cycle-closing chains; rows[2i], rows[2i+1]
 * = the flux end row and the multiplier row whose coupling that drops (precond.py
 * TreePreconditioner.cyc_rows). The tree solve inverts A without those n symmetric +-1
 * pairs; nx_solve adds them back with a rank-2n Woodbury correction built once per assembled
 * matrix (2n tree solves of unit vectors, a (2n)^2 capacitance matrix), then checks the true
 * residual with the CSR. n <= 128 (else the solve runs MINRES); n = 0 clears it. Set after
 * every nx_set_preconditioner (which clears it). Replaces nothing one-to-one: MUMPS'
 * factorisation (solver.py:58-65) covers cycles implicitly.
 */
int nx_set_cycles(nx_network_t* h, int32_t n, const int32_t* rows);
/* The same correction with several ranks (RCCL ranks or an in-process group): every rank
 * calls it after nx_set_preconditioner with the cycle chains of ALL ranks in one global
 * order (K pairs, K <= 128; the host control plane gathers them). own[2K]: per column of U
 * (pair k's flux end at 2k, its multiplier at 2k + 1) this rank's row, or -1 where another
 * rank owns it; qloc[K] / lcol[K]: for the pairs whose chain is this rank's, the flux end row
 * and the multiplier's column in this rank's numbering (a ghost column when another rank
 * owns the multiplier row), else -1. Z = A_g^{-1} U is built by 2K team tree solves, U^T Z
 * and the couplings are summed over the ranks (one all-reduce), every rank inverts the same
 * capacitance matrix; per solve U^T x is summed (one all-reduce of 2K), x -= Z Cinv U^T x on
 * every rank's rows, and the true residual comes from the CSR after a halo of x. The cycle
 * count is part of the ranks' schedule signature. K = 0 clears it. Replaces MUMPS'
 * distributed factorisation of a cyclic graph (solver.py:58-65, mesh.py:341-348). */
int nx_set_cycles_team(nx_network_t* h, int32_t K, const int32_t* own, const int32_t* qloc,
                       const int32_t* lcol);

/*
 * General flux degree k >= 2 with DG0 pressure (assembly.py:121-146, flux_degree=k), one
 * rank: the direct solve through the condensed system. The DG0 divergence touches a cell's
 * two vertex fluxes only, so the k-1 interior fluxes per cell are condensed out per cell;
 * what remains has the P1/DG0 structure with the cell mass R h [[a, b], [b, a]]
 * (element.condensed_flux_mass: k = 2: a = 1/8, b = -1/24). An auxiliary P1/DG0 handle of
 * the same graph (nx_create + its tree preconditioner, nx_set_solver 1) inverts it.
 *
 * nx_set_cell_mass(aux, ratio, mo_div): the auxiliary handle's flux mass is the condensed
 *   one, ratio = a / b (T = tridiag(1, 2 ratio, 1), ratio at both ends; P1: 2) and mo_div =
 *   (a + b) / b (P1: 3). The handle is internal from then on: its own CSR is no longer the
 *   system its sweeps invert (it checks no residual; nx_solve on it runs MINRES).
 * nx_fe_set_direct(h, aux, k, n_lm, ...): attaches aux to the (k, 0) handle h (nx_create_fe):
 *   slot[e] = aux edge of h's edge e; v_fe / v_aux (E (N+1)) the vertex-flux rows, edge-major;
 *   i_fe (E N (k-1)) the interior-flux rows, cell-major; p_fe / p_aux (E N) pressure rows;
 *   l_fe / l_aux (n_lm) multiplier rows; cst = C (2 x (k-1)) | K ((k-1) x 2) | M_ii^{-1}
 *   ((k-1)^2) | the reference flux mass ((k+1)^2, node order along the cell; what
 *   nx_fe_batch_gradient contracts with), row-major; ab = a + b. aux = NULL detaches.
 *   With nx_set_solver(h, 1, 1), nx_solve condenses, solves on aux, expands, checks h's true residual and refines up to
 *   twice (iters = passes), MINRES when that still misses rtol. layout_fe.build_fe_aux_maps
 *   builds the maps. Replaces MUMPS' LU of the (k, 0) system (solver.py:58-65).
 *   Several ranks: h (n_ghost > 0) and aux (the rank's P1/DG0 handle with its halo, cut rows
 *   and preconditioner) each joined to the ranks' communicator; the aux solve is the ranks'
 *   direct tree solve, h's residual takes the halo of x and one all-reduce.
 */
int nx_set_cell_mass(nx_network_t* aux, double ratio, double mo_div);
int nx_fe_set_direct(nx_network_t* h, nx_network_t* aux, int32_t k, int64_t n_lm,
                     const int32_t* slot, const int32_t* v_fe, const int32_t* v_aux,
                     const int32_t* i_fe, const int32_t* p_fe, const int32_t* p_aux,
                     const int32_t* l_fe, const int32_t* l_aux, const double* cst, double ab);

/*
 * Continuous pressure (pressure_degree m >= 1, flux_degree k > m; assembly.py:121-146), one
 * rank, a forest: the direct solve by condensation onto the graph nodes, replacing MUMPS'
 * LU (solver.py:58-65) for these pairs. Each edge's own unknowns (its kN+1 flux nodes and
 * mN-1 interior pressure nodes) are eliminated onto its border: the pressure at its two end
 * nodes (shared with the other edges there) and the multipliers of the bifurcations at its
 * ends. Per cell the interior nodes condense onto the vertices by exact reference blocks
 * scaled by s = R h (layout: element.condensed_cell_blocks); per edge the vertices (q, p)
 * are eliminated along it (one thread per edge); the border system over the graph nodes
 * (negative definite, 2 unknowns per node) is eliminated leaf to root by one workgroup;
 * then every edge back-substitutes. The true residual comes from the CSR, with up to two
 * refinement passes; nx_get_direct_path reports 4.
 *   nI = (k-1)+(m-1); cst = Kh (16) | Ch (4 nI) | Eh (4 nI) | Fh (nI nI) | the reference flux
 *   mass ((k+1)^2, node order along the cell, row-major) | the m + 1 source weights of a cell's
 *   pressure rows per unit f h, the layout's sign included (the last two are what
 *   nx_cp_batch_gradient contracts with); tI[nI] (+1 flux,
 *   -1 pressure interior node); n_nodes border nodes, nrow[2n] (pressure row, multiplier row
 *   or -1); eb[4E] (source node, target node, the q_0 - lam_source and q_N - lam_target
 *   couplings: 0 or +-1); the node forest: n_lev levels (lev_off, order), every node's
 *   (edge, end) incidences (inc_off, inc), parent[3n] (parent node, edge, this node's end of
 *   it; -1 at a root), children (child_off, child), nown[n] (the edge that writes the node's
 *   rows). k = 0 detaches it. Built by layout_fe.build_cp_tables.
 */
int nx_fe_set_cp(nx_network_t* h, int32_t k, int32_t m, int32_t nI, const double* cst,
                 const int32_t* tI, int64_t n_nodes, const int32_t* nrow, const int32_t* eb,
                 int32_t n_lev, const int32_t* lev_off, const int32_t* order,
                 const int32_t* inc_off, const int32_t* inc, const int32_t* parent,
                 const int32_t* child_off, const int32_t* child, const int32_t* nown);

/*
 * Several ranks, continuous pressure (called before nx_fe_set_cp; layout_fe.
 * build_cp_rank_tables): this rank runs the edge kernels on its n_own_edges edges (gid: each
 * one's global edge), every rank's border blocks and the node rows' rhs are summed over the
 * ranks (one all-reduce per pass), every rank solves the node forest, and each writes the
 * node rows it owns (nrowx, 2 per node: local rows or -1). nx_fe_set_cp's eb / nown then
 * list this rank's edges (nown: -1 where another rank writes the node), its nrow the node
 * rhs slots (2n, 2n + 1 or -1), its incidence and parents global edges. Replaces the
 * distributed MUMPS LU (solver.py:58-65) for these pairs.
 */
int nx_fe_cp_ranks(nx_network_t* h, int64_t n_own_edges, int64_t n_edges_global,
                   const int32_t* gid, int64_t n_nodes, const int32_t* nrowx);

/*
 * Continuous pressure on a graph with cycles (called after nx_fe_set_cp, whose parents and
 * levels then describe a BFS spanning forest while its incidences keep every edge;
 * layout_fe.build_cp_tables(cycles=True)): the n_chords non-tree edges (chord, ascending
 * edge ids -- global ones on several ranks) and the n_slots distinct real border slots at
 * their ends (cslot, 2 per slot: node, 0 pressure / 1 multiplier; sorted; the multiplier
 * only where the node has one). The forest's elimination then inverts the grounded node
 * system S_g (S minus every chord's two off-diagonal 2 x 2 border blocks; negative definite
 * like S), and the solve corrects it: S = S_g + U C U^T, x = S_g^-1 (g - U w) with
 * w = (I + C U^T Z)^-1 C U^T x_g, Z = S_g^-1 U. The n_slots x n_slots capacitance matrix is
 * built and inverted on the device once per contents of R (new boundary values or a new
 * source do not rebuild it); per pass the node sweep runs three times (x_g, the corrected
 * solve, one refinement of it). Several ranks need no
 * further communication: every rank forms the same matrix from the summed blocks. A
 * singular capacitance matrix detaches the correction (the solves run MINRES).
 * NX_ERR_ARG: n_slots above 4096 (2 kMaxCyc), indices out of range, a chord that is a
 * forest edge. n_chords = 0 clears it. Replaces MUMPS' LU (solver.py:58-65) of these pairs
 * on the graphs it factorises and the forest solve did not (the reference's own cyclic
 * graph, tests/test_edge_info.py:8-35).
 */
int nx_fe_cp_set_cycles(nx_network_t* h, int32_t n_chords, const int32_t* chord,
                        int32_t n_slots, const int32_t* cslot);
/* The chords' correction (nx_fe_cp_set_cycles): *ran = 1 when the last node-condensed solve
 * applied it; *builds = how many times this handle has built its capacitance matrix. Either
 * pointer may be NULL. Replaces nothing in the reference. */
int nx_get_cp_cycles(nx_network_t* h, int32_t* ran, int32_t* builds);

/*
 * Process-wide solve mode. 1 (default): with the preconditioner a solve is ONE HIP graph
 * launch -- start application, per-solve coefficients and the first iterations (also with
 * several ranks, RCCL or group, when beta^2 travels point-to-point) -- whose last k_mr_a
 * publishes the MINRES state to host-coherent memory; nx_solve returns once it is
 * published (the final solution update may still run: every host read of device data
 * synchronises the stream). 0: eager prologue, chunked iteration graphs, a stream
 * synchronisation per chunk (the path profiling always uses). NXHIP_LEAN=0 sets 0.
 */
int nx_set_lean(int32_t enable);

/*
 * Coarse step of the preconditioner on a partitioned problem (precond.py derives it): the
 * coarse junctions (interface junctions + the junctions on paths between them inside a
 * rank) form a forest that every rank solves redundantly from one all-reduce of
 * [D | J | G] (3 n_coarse doubles) per application, which keeps P^{-1} exact, i.e. the
 * iteration count independent of the number of ranks.
 *   slot_cidx[n_slots]        coarse index of every slot, -1 (coarse slots: top part)
 *   cc_chain/cc_top/cc_bot    local chains joining two coarse junctions: chain, coarse
 *                             index of its top / bottom end (the bottom is the child)
 *   c_parent[n_coarse], c_child_off/c_child (CSR), c_lvl_off[n_clvl+1]: the global
 *                             forest in level order (root level first)
 * n_coarse = 0 disables the step. Call after nx_set_preconditioner.
 */
int nx_set_coarse(nx_network_t* h, int32_t n_coarse, const int32_t* slot_cidx, int32_t n_cc,
                  const int32_t* cc_chain, const int32_t* cc_top, const int32_t* cc_bot,
                  const int32_t* c_parent, const int32_t* c_child_off, const int32_t* c_child,
                  int32_t n_clvl, const int32_t* c_lvl_off);

/* 1 if the last nx_solve replayed its iterations as HIP graphs (also with RCCL, unless
 * the capture failed or NXHIP_RCCL_GRAPH=0), 0 if it launched them one by one. */
int nx_get_graph_mode(nx_network_t* h, int32_t* graph);

/*
 * Many boundary / source scenarios against the handle's current matrix in one batched pass
 * of the direct solve. The reference answers one scenario per KSP solve (solver.py:107-135)
 * and would loop compute_forms + assemble + solve (assembly.py:165-262, 329-368); here the
 * matrix depends on R and the geometry alone, a scenario changes the right-hand side only,
 * and the sweeps get a column dimension (k_b_*: grid = jobs x columns).
 *
 * nx_batch_supported: *ok = 1 when nx_batch_solve would take the batched kernels on this
 * handle, else 0: an nx_create (P1/DG0) handle, one rank, not in a group,
 * nx_set_solver(h, 1, .), the exact preconditioner, the LDS sweeps, and tree_exact or a
 * cycle correction (nx_set_cycles). Anything else makes nx_batch_solve return NX_ERR_STATE.
 *
 * nx_batch_solve: n_cols scenarios.
 *   edge_bc   n_cols x E x 2 (as nx_set_coefficients' edge_bc)
 *   edge_f    n_cols x E, or NULL
 *   f_const   n_cols, or NULL (then the handle's source); ignored where edge_f is given
 *   order     0 device layout, 1 the output map (NX_ERR_STATE if none was set)
 *   out       n_cols x n_rows; iters / relres / converged: n_cols each (any may be NULL)
 * A pending deferred assembly is flushed first; the matrix must have been assembled. The
 * lumped mass and, on a graph with cycles, the correction are made current for the matrix
 * (nothing current is rebuilt). The handle's coefficients, rhs, x, tmp, published state and
 * snapshots are left as they were. Columns go in chunks of NXHIP_BATCH_CHUNK (read per call)
 * or the largest of <= 64 whose workspace fits a quarter of the free device memory; the
 * workspace is allocated on first use and freed by nx_destroy (a failed allocation halves
 * the chunk down to 1 before NX_ERR_HIP). Per column: solve, true residual
 * ||b - A x|| / ||b|| against the CSR, one refinement pass for the columns above rtol (a
 * list of those columns only), then the single-column nx_solve path (with its MINRES) for a
 * column still above it. b = 0 gives x = 0, relres = 0, converged = 1. A column's bits do
 * not depend on the other columns, its position, n_cols or the chunk size.
 * NX_ERR_ARG: n_cols < 1, NULL edge_bc / out.
 *
 * nx_batch_rhs (test hook): only the batched rhs kernel; out = n_cols x n_rows, device
 * layout, every column bit-equal to nx_assemble's rhs of that scenario.
 *
 * nx_get_batch_info: the last nx_batch_solve's kernel launches -- its batched passes (7 per
 * chunk on a forest, 9 with cycles; 6 / 8 more for a chunk with a refinement pass) and what it had
 * to make current first (1 for a flushed assembly, 1 for the lumped mass, and the whole build
 * of the cycle correction: 2 n_cyc unit solves and the inversion), so a call that found
 * everything current reports the passes alone; the launches inside a column's single-column
 * fallback are not counted -- then the columns that took the refinement pass, the columns
 * handed to the single-column path, and the chunk size used.
 */
int nx_batch_supported(nx_network_t* h, int32_t* ok);
int nx_batch_solve(nx_network_t* h, int32_t n_cols, const double* edge_bc,
                   const double* edge_f, const double* f_const, double rtol, int32_t order,
                   double* out, int32_t* iters, double* relres, int32_t* converged);
int nx_batch_rhs(nx_network_t* h, int32_t n_cols, const double* edge_bc, const double* edge_f,
                 const double* f_const, double* out);
int nx_get_batch_info(nx_network_t* h, int32_t* launches, int32_t* refined, int32_t* fallback,
                      int32_t* chunk);

/*
 * nx_batch_solve for flux degree k >= 2 with DG0 pressure: many boundary / source scenarios
 * against the current matrix of a (k, 0) handle in one batched pass of its condensed direct
 * solve (nx_fe_set_direct). The reference answers one scenario per KSP solve
 * (solver.py:107-135) and would loop compute_forms + assemble + solve; here the per-cell
 * condensation, the auxiliary P1/DG0 tree sweeps and the expansion get a column dimension.
 *
 * nx_fe_batch_supported: *ok = 1 when nx_fe_batch_solve takes the batched kernels on this
 * handle, else 0: an nx_create_fe handle with pressure degree 0 and an auxiliary handle
 * attached (nx_fe_set_direct), one rank, not in a group, no ghosts, nx_set_solver(h, 1, 1), and
 * the auxiliary handle with the exact preconditioner, the LDS sweeps, and tree_exact or a cycle
 * correction. Continuous-pressure and P1/DG0 handles give 0 (and nx_batch_supported stays 0
 * for every nx_create_fe handle).
 *
 * nx_fe_batch_solve: n_cols scenarios; edge_bc / edge_f / f_const / rtol / order / out /
 * iters / relres / converged as nx_batch_solve, out = n_cols x n_rows of the (k, 0) handle;
 * maxit caps the MINRES of a column's single-column fallback. NX_ERR_STATE where
 * nx_fe_batch_supported says 0, where the matrix has not been assembled for the resident
 * coefficients, or order != 0 without an output map; NX_ERR_ARG as nx_batch_solve (and
 * maxit < 1). A pending deferred assembly is flushed first.
 * Per chunk (the chunk rule is nx_batch_solve's; the workspace is the (k, 0) columns' plus the
 * auxiliary system's, allocated on first use, freed by nx_destroy and when nx_fe_set_direct
 * detaches; per column 4 n_rows + 2 n_aux + 3 E + 5 slots + 2 n_cyc doubles and the inputs):
 *   k_fe_b_rhs        every column's rhs from the rhs gather tables, k_assemble_fe's terms in
 *                     its order: bit-equal to nx_assemble's rhs of that scenario
 *   k_fe_b_condense   b_v - C b_i on the vertex rows, pressure / multiplier rows copied, into
 *                     the auxiliary columns; the auxiliary lumped mass (a + b) R h once per call
 *   k_b_up / k_b_top / k_b_down with the auxiliary handle's decomposition, on this handle's
 *                     stream; with cycles k_cyc_w / k_cyc_fix with the auxiliary Z / Cinv,
 *                     built first (cyc_build) where the matrix is new
 *   k_fe_b_expand     the (k, 0) solution; added in a refinement pass
 *   k_b_res / k_b_norms   the true residual against this handle's CSR
 *   k_b_gather        when order != 0, then one copy per chunk
 * Per column the policy is nx_batch_solve's: one refinement pass over the list of columns above
 * rtol, then the handle's single-column route (fe_solve_direct, then MINRES capped at maxit)
 * for a column still above it -- where that route ends unconverged with a residual no better
 * than the refined column's (its MINRES is unpreconditioned and starts from zero), the refined
 * column stands, with its residual and converged = 0; b = 0 gives x = 0, relres = 0,
 * converged = 1. A column's bits do
 * not depend on the other columns, its position, n_cols or the chunk size. The handle's
 * coefficients, rhs, x, tmp, published state and snapshots are left as they were.
 *
 * Launches (nx_get_batch_info reports the last nx_fe_batch_solve as it does nx_batch_solve's):
 * per chunk 9 on a forest -- rhs, condense, up, top, down, expand, residual, norms, gather -- 7
 * where the decomposition has no subtree jobs (no up / down), 11 / 9 with cycles; 8 / 6 / 10 / 8
 * with order = 0 (no gather). A chunk with a refinement pass adds 7 (5 without jobs), 9 (7)
 * with cycles. What the call had to make current first is counted too: 1 for a flushed
 * assembly and the whole build of the cycle correction.
 *
 * nx_fe_batch_rhs (test hook): k_fe_b_rhs alone; out = n_cols x n_rows, device layout.
 */
int nx_fe_batch_supported(nx_network_t* h, int32_t* ok);
int nx_fe_batch_solve(nx_network_t* h, int32_t n_cols, const double* edge_bc,
                      const double* edge_f, const double* f_const, double rtol, int32_t maxit,
                      int32_t order, double* out, int32_t* iters, double* relres,
                      int32_t* converged);
int nx_fe_batch_rhs(nx_network_t* h, int32_t n_cols, const double* edge_bc, const double* edge_f,
                    const double* f_const, double* out);

/*
 * nx_batch_solve for continuous pressure (k > m >= 1) on a forest: many boundary / source
 * scenarios against the current matrix in one batched pass of the node-condensed direct solve
 * (nx_fe_set_cp). The single solve factors the matrix again on every pass of every scenario;
 * here what depends on the matrix alone is formed once per call and a chunk of columns sweeps
 * its right-hand sides only.
 *
 * nx_cp_batch_supported: *ok = 1 when nx_cp_batch_solve takes the batched kernels on this
 * handle, else 0: an nx_create_fe handle with the node-condensed solve attached
 * (nx_fe_set_cp), nx_set_solver(h, 1, 1), one rank (no nx_fe_cp_ranks, not in a group, no
 * ghosts), at least one edge, and no chords attached (nx_fe_cp_set_cycles) -- or chords and
 * nx_set_cp_batch_cycles(h, 1), below. (k, 0) and P1/DG0 handles give 0.
 *
 * nx_cp_batch_solve: the arguments of nx_fe_batch_solve; out = n_cols x n_rows. NX_ERR_STATE
 * where nx_cp_batch_supported says 0, where the matrix has not been assembled for the
 * resident coefficients, or order != 0 without an output map; NX_ERR_ARG as nx_batch_solve
 * (and maxit < 1). A pending deferred assembly is flushed first.
 * Once per call (the factor stage; it writes the batch's workspace alone):
 *   k_cp_b_factor     k_cp_edge's sweep without a right-hand side: per vertex the pivot
 *                     inverse and couplings Pi | C | W (16 doubles, cp_fac's edge-minor
 *                     layout), per edge the 4 x 4 border block Se
 *   the node forest's up-sweep of the single solve (k_cp_nodes / k_cp_nodes_rec / k_cp_level)
 *                     on those blocks and a zero right-hand side: every node's pivot inverse
 * Per chunk (the chunk rule is nx_batch_solve's; a grid covers columns as well as edges or
 * nodes, kCpTile = 4 columns per work item):
 *   k_fe_b_rhs        every column's rhs, bit-equal to nx_assemble's rhs of that scenario
 *   k_cp_b_fwd        per edge: the cells' interior rhs condensed onto the vertices, the rho
 *                     chain; z = Pi rho per vertex and ge per edge, per column
 *   k_cp_b_nodes / k_cp_b_level   the node forest on right-hand sides only, up (h_n = b rows +
 *                     sum ge - the children's terms; the node's own term B^T P^-1 h_n) and
 *                     down (x_n = P_n^-1 (h_n - B x_parent)), over the single solve's level runs
 *   k_cp_b_back       per edge: the vertex recursion and the cells' interiors into the chunk's
 *                     columns (added in a refinement pass); the node rows by cp_nown's edge
 *   k_b_res / k_b_norms   the true residual against this handle's CSR
 *   k_b_gather        when order != 0, then one copy per chunk
 * The workspace is the handle's columns (nx_batch_solve's) plus, owned by the handle, the
 * call's factors (16 (N + 1) E + 20 E + 12 nodes + n_rows doubles) and per column
 * 2 (N + 1) E + 4 E + 6 nodes doubles; allocated on first use, freed by nx_destroy and by
 * nx_fe_set_cp. The handle's own factors, node arrays, coefficients, rhs, x, tmp, published
 * state and snapshots are left as they were.
 * Per column the policy is nx_fe_batch_solve's: one refinement pass over the columns above
 * rtol, then the single-column route (fe_cp_solve, then MINRES capped at maxit), the refined
 * column standing where that ends unconverged and no better; b = 0 gives x = 0, relres = 0,
 * converged = 1. A column's bits do not depend on the other columns, its position, n_cols or
 * the chunk size.
 *
 * Launches (nx_get_batch_info): F + chunks x S, plus 1 for a flushed assembly. With U / D the
 * launches of the node forest's up / down pass -- one per run of levels: U = D = 1 where no
 * level of the forest holds more than 128 nodes -- the factor stage is F = 1 + U and a chunk
 * is S = 6 + U + D with order != 0 (rhs, forward, up, down, back, residual, norms, gather),
 * 5 + U + D with order = 0, whatever its column count. A chunk with a refinement pass adds
 * 4 + U + D.
 *
 * Graphs with cycles (nx_set_cp_batch_cycles; off by default). With chords attached
 * (nx_fe_cp_set_cycles) the factor stage above factors the grounded system S_g, and every
 * column takes the single solve's correction on the batch's own factors,
 *   x = S_g^-1 (g - U w),   w = (I + C U^T Z)^-1 C U^T x_g,   x_g = S_g^-1 g,
 * with one refinement of the grounded solve. Once per contents of R (kept across calls; new
 * boundary values or sources build nothing): U^T Z (k_cp_zcols), I + C U^T Z (k_cp_cap) and its
 * inverse (k_gj_*) on the call's factors into an ns x ns array the batch owns (ns the border
 * slots at chord ends, at most 4096; allocated when the switch is set and chords are attached,
 * freed with the chord tables) -- never the single solve's inverse: the two factor sets differ
 * in their last bits, and a shared inverse would make a solve's bits depend on the batched calls
 * before it. The handle's Gauss-Jordan array and column scratch serve the build. Per chunk,
 * between the node forest's down pass and k_cp_b_back, each with grid = (work, column tiles):
 *   k_cp_b_cyc_w      y = C U^T x_g per column in LDS, then w = Inv y: a workgroup takes 64 rows
 *                     of Inv against a tile of 4 columns, each element of Inv read once per
 *                     tile; a row's sum in 8 strided parts joined in order, no contraction
 *                     (LDS 32 ns + 16 K bytes: 144 KB at 4096 slots)
 *   k_cp_b_cyc_rhs    the node right-hand side g - U w (2 per node: 2 n, 2 n + 1)
 *   k_cp_b_nodes<1> / k_cp_b_level<1>   the forest up and down on that right-hand side
 *   k_cp_b_cyc_res    the grounded system's node residual of the result
 *   k_cp_b_nodes<1> / k_cp_b_level<1>   the forest on the residual
 *   k_cp_b_cyc_add    x_n += the sweep's values
 * so every solve pass -- a chunk's first and its refinement -- adds 4 + 2 (U + D): S = 10 + 3 (U +
 * D) with order != 0 and a refinement pass 8 + 3 (U + D). The call that builds the inverse adds
 * ceil(ns / b) + 2 ns + 2, b the column batch of nx_fe_cp_set_cycles (min(ns, 512) unless the
 * forest has more than 32768 nodes). Per column the workspace grows by ns + 6 nodes doubles. A
 * zero pivot in the build marks the batch's correction failed: nx_cp_batch_supported says 0
 * from then on, and that call's columns miss the residual check and take the single-column
 * route. A failed allocation of the inverse leaves nx_cp_batch_supported at 0.
 *
 * nx_set_cp_batch_cycles: handle state, enable = 0 / 1 (NX_ERR_ARG otherwise, and for a NULL
 * handle). It may be set before or after the chords are attached. Without it a handle with
 * chords says 0 to nx_cp_batch_supported, as before.
 * nx_get_cp_batch_cycles: the flag, whether the last nx_cp_batch_solve / nx_cp_batch_gradient
 * applied the correction, and the batch's own builds of the inverse so far (NULL outputs are
 * skipped). nx_get_cp_cycles's figures are the single solve's and do not move with the batch.
 *
 * nx_cp_batch_rhs (test hook): k_fe_b_rhs alone; out = n_cols x n_rows, device layout.
 */
int nx_cp_batch_supported(nx_network_t* h, int32_t* ok);
int nx_set_cp_batch_cycles(nx_network_t* h, int32_t enable);
int nx_get_cp_batch_cycles(nx_network_t* h, int32_t* enabled, int32_t* applied,
                           int32_t* builds);
int nx_cp_batch_solve(nx_network_t* h, int32_t n_cols, const double* edge_bc,
                      const double* edge_f, const double* f_const, double rtol, int32_t maxit,
                      int32_t order, double* out, int32_t* iters, double* relres,
                      int32_t* converged);
int nx_cp_batch_rhs(nx_network_t* h, int32_t n_cols, const double* edge_bc, const double* edge_f,
                    const double* f_const, double* out);

/*
 * Adjoint gradients of an observed-row objective with respect to every edge's R, every
 * boundary value and every edge's source, for n_cols scenarios, in two batched direct solves;
 * no solution leaves the device (the reference has no counterpart). Per scenario j over the
 * observed device rows r_i (distinct) with weights w_i:
 *   kind 1 (least squares)  J_j = 1/2 sum_i w_i (x_j[r_i] - d_ji)^2
 *   kind 0 (linear)         J_j = sum_i w_i x_j[r_i]
 * The device system is symmetric (its pressure rows are the reference's, negated), so the
 * adjoint system is the same matrix with the right-hand side c_j = dJ_j/dx -- w_i
 * (x_j[r_i] - d_ji), or w_i -- and goes through the same batched sweeps, cycle correction,
 * residual check, refinement pass and single-column fallback as nx_batch_solve's columns;
 * c = 0 gives a zero adjoint, converged. Kind 0 has one adjoint column for all scenarios: it
 * is solved once per call. With mu = A^{-1} c and x the forward solution (both stay resident
 * in the workspace, which grows by two vectors and 4 E + 1 outputs per column):
 *   grad_R[j, e]     = -sum_k h_k/6 (2 mu_k x_k + mu_k x_{k+1} + mu_{k+1} x_k + 2 mu_{k+1} x_{k+1})
 *                      over the edge's cells (its flux vertex values: the R = 1 P1 mass)
 *   grad_bc[j, e, .] = mu at the edge's q_0 / q_N row: the derivative w.r.t. edge_bc[j, e, .]
 *   grad_f[j, e]     = -sum_k h_k mu[p_k]: the derivative w.r.t. the edge's source
 * (the derivatives w.r.t. what the caller passes: edge slots, edge_bc with the sign
 * nx_set_coefficients documents).
 *   edge_bc / edge_f / f_const / rtol   as nx_batch_solve
 *   obs_rows, obs_w   n_obs each; obs_d  n_cols x n_obs (NULL for kind 0)
 *   value   n_cols;  grad_R  n_cols x E;  grad_bc  n_cols x E x 2 or NULL;  grad_f  n_cols x E
 *   or NULL;  iters / relres / converged  2 x n_cols each or NULL: the forward columns, then
 *   the adjoint columns (kind 0: its one column's figures for every scenario)
 * Supported exactly where nx_batch_supported says 1, else NX_ERR_STATE. It makes current what
 * nx_batch_solve makes current and leaves the handle's coefficients, rhs, x, tmp, published
 * state and snapshots as they were; chunks as nx_batch_solve (NXHIP_BATCH_CHUNK, <= 64, a
 * quarter of the free memory with the larger columns). A column's bits do not depend on the
 * other columns, its position, n_cols or the chunk size. Per chunk one device-to-host copy per
 * output array, straight into the caller's memory (page-locked memory makes each one DMA):
 * (4 E + 1) doubles per column in all.
 * NX_ERR_ARG: n_cols < 1, n_obs < 1, a row outside [0, n_rows), duplicate rows, an unknown
 * kind, kind 1 without obs_d, NULL edge_bc / value / grad_R / obs_rows / obs_w.
 *
 * nx_get_batch_info then reports this call (refined: forward plus adjoint columns). Steady
 * launches when nothing is refined, with S = 5 on a forest (up, top, down, residual, norms)
 * and S = 7 with cycles (the correction's two kernels):
 *   kind 1   per chunk  1 (rhs) + S + 1 (k_b_obs) + S + 1 (k_b_edge_form): 13 / 17
 *   kind 0   per call   1 (k_b_obs) + S: 6 / 8;  per chunk  1 + S + 1 + 1: 8 / 10
 * and 6 / 8 more for each refinement pass, as nx_batch_solve.
 */
int nx_batch_gradient(nx_network_t* h, int32_t n_cols, const double* edge_bc,
                      const double* edge_f, const double* f_const, double rtol, int32_t kind,
                      int32_t n_obs, const int32_t* obs_rows, const double* obs_w,
                      const double* obs_d, double* value, double* grad_R, double* grad_bc,
                      double* grad_f, int32_t* iters, double* relres, int32_t* converged);

/*
 * nx_fe_batch_gradient: nx_batch_gradient for flux degree k >= 2 with DG0 pressure, on the
 * (k, 0) handle's batched condensed solve (nx_fe_batch_solve's operator: condense, the
 * auxiliary sweeps with their cycle correction, expand). The (k, 0) device matrix is symmetric
 * too, so the adjoint is the same solve with k_b_obs's right-hand side. Objectives, arguments,
 * outputs, status arrays (2 x n_cols: forward, then adjoint), the once-per-call adjoint column
 * of kind 0 and the exact zeros of a zero right-hand side are nx_batch_gradient's; maxit caps
 * the MINRES of a column's single-column fallback, as in nx_fe_batch_solve, whose per-column
 * policy both passes follow. obs_rows are device rows of the (k, 0) handle: any flux node
 * (vertex or interior), pressure or multiplier row. With mu = A^{-1} c and x the forward
 * solution, per edge over its N cells c (length h_c; x_c, mu_c the cell's k + 1 flux node
 * values, left vertex, interior, right vertex; M the (k+1) x (k+1) reference mass):
 *   grad_R[j, e]     = -sum_c h_c mu_c^T M x_c     (-mu^T (dA/dR_e) x: A is affine in R and only
 *                      its flux-flux block depends on it)
 *   grad_f[j, e]     = sum_c (h_c v) mu[p_c], v the source term of the pressure row p_c in the
 *                      rhs tables (DG0: v = -1, so -sum_c h_c mu[p_c])
 *   grad_bc[j, e, .] = mu at the edge's first / last flux vertex row
 * k_fe_b_edge_form forms them per (column, edge), addressing rows through nx_fe_set_direct's
 * maps, in k_b_edge_form's lane shapes; M is part of the handle's constants (nx_fe_set_direct)
 * and staged in LDS per workgroup. Fixed-order sums, no contraction: a column's bits do not
 * depend on the other columns, its position, n_cols or the chunk size.
 * Supported exactly where nx_fe_batch_supported says 1, else NX_ERR_STATE; NX_ERR_STATE too
 * where the matrix has not been assembled for the resident coefficients. NX_ERR_ARG:
 * nx_batch_gradient's cases, and maxit < 1. The workspace is nx_fe_batch_solve's with the
 * gradient's part (two more vectors and 4 E + 1 outputs per (k, 0) column); a workspace that an
 * earlier nx_fe_batch_solve allocated without it is allocated again with it, and keeps it.
 * The first pass of a call writes the auxiliary lumped mass and makes the auxiliary cycle
 * correction current (kind 0: the one adjoint column's pass, which runs before any forward
 * pass). The handle's coefficients, rhs, x, tmp, published state and snapshots are left as
 * they were. Not served: Hessian-vector products, ensembles (a resistance field per scenario)
 * and several ranks; continuous pressure (m >= 1) has its own entry, nx_cp_batch_gradient.
 *
 * Launches (nx_get_batch_info reports the call; refined: forward plus adjoint columns). Let P
 * be the launches of one solve pass without rhs and gather -- condense, s sweeps, expand,
 * residual, norms -- with s = 3 where the auxiliary decomposition has subtree jobs, else 1:
 * P = s + 4, and s + 6 with cycles (the correction's two kernels). Steady, nothing refined:
 *   kind 1   per chunk  1 (rhs) + P + 1 (k_b_obs) + P + 1 (k_fe_b_edge_form)
 *   kind 0   per call   1 (k_b_obs) + P;  per chunk  1 + P + 1 + 1
 * A refinement pass adds P, what it adds in nx_fe_batch_solve (7, 5 without jobs; 9, 7 with
 * cycles). What the call had to make current is counted as there: 1 for a flushed
 * assembly and the whole build of the cycle correction.
 */
int nx_fe_batch_gradient(nx_network_t* h, int32_t n_cols, const double* edge_bc,
                         const double* edge_f, const double* f_const, double rtol, int32_t maxit,
                         int32_t kind, int32_t n_obs, const int32_t* obs_rows, const double* obs_w,
                         const double* obs_d, double* value, double* grad_R, double* grad_bc,
                         double* grad_f, int32_t* iters, double* relres, int32_t* converged);

/*
 * nx_cp_batch_gradient: nx_batch_gradient for continuous pressure (k > m >= 1) on a forest, on
 * the handle's batched node-condensed solve (nx_cp_batch_solve's factor stage and operator).
 * The device matrix of every general-degree layout is symmetric (pressure rows negated), so the
 * adjoint is the same solve with k_b_obs's right-hand side. Objectives, arguments, outputs,
 * status arrays (2 x n_cols: forward, then adjoint), the once-per-call adjoint column of kind 0
 * and the exact zeros of a zero right-hand side are nx_batch_gradient's; maxit caps the MINRES
 * of a column's single-column fallback, as in nx_cp_batch_solve, whose per-column policy both
 * passes follow. obs_rows are device rows of the (k, m) handle: any flux node, edge-interior
 * pressure node, node pressure or multiplier row. With mu = A^{-1} c and x the forward
 * solution, per edge over its N cells c (length h_c):
 *   grad_R[j, e]     = -sum_c h_c mu_c^T M x_c   (x_c, mu_c the cell's k + 1 flux node values,
 *                      local rows k c .. k c + k; M the (k+1) x (k+1) reference mass: A is
 *                      affine in R and only its flux-flux block depends on it)
 *   grad_f[j, e]     = sum_c h_c sum_{i=0..m} s_i mu[p_{c,i}]   (p_{c,i} the cell's m + 1 pressure
 *                      rows, the first of cell 0 and the last of cell N - 1 being the node rows
 *                      of the edge's end nodes -- a node row shared by several edges counts this
 *                      edge's cells only; s_i what k_fe_b_rhs puts into that row per unit f h_c)
 *   grad_bc[j, e, .] = mu at the edge's first / last flux row (local rows 0 and k N)
 * k_cp_b_edge_form forms them per (column, edge) in k_b_edge_form's lane shapes; the rows are in
 * closed form (edge e's block starts at e ((k + m) N), flux node j is local row j, interior
 * pressure node j local row k N + j, the end nodes' pressure rows nrow[2 u] / nrow[2 v]); M and
 * s are part of the handle's constants (nx_fe_set_cp, behind Fh) and staged in LDS per
 * workgroup. Fixed-order sums, no contraction: a column's bits do not depend on the other
 * columns, its position, n_cols or the chunk size.
 * Supported exactly where nx_cp_batch_supported says 1, else NX_ERR_STATE; NX_ERR_STATE too
 * where the matrix has not been assembled for the resident coefficients. NX_ERR_ARG:
 * nx_batch_gradient's cases, and maxit < 1. Once per call the factor stage of nx_cp_batch_solve
 * runs (it depends on the resident R alone) and serves the forward pass, the adjoint pass and
 * their refinements; kind 0 then solves its one adjoint column, before any forward pass. The
 * workspace is nx_cp_batch_solve's with the gradient's part (two more vectors and 4 E + 1
 * outputs per column); a workspace that an earlier nx_cp_batch_solve allocated without it is
 * allocated again with it, and keeps it. The handle's own factors, coefficients, rhs, x, tmp,
 * published state and snapshots are left as they were. Not served: Hessian-vector products,
 * ensembles (a resistance field per scenario), several ranks, and graphs with cycles unless the
 * handle has opted in (nx_set_cp_batch_cycles): the correction is part of the symmetric
 * operator, so the forward pass, the adjoint pass and their refinements all go through the
 * corrected solve, and every edge -- chords included -- contributes to the contraction through
 * its own rows. The inverse is built at most once per call, before kind 0's adjoint column.
 *
 * Launches (nx_get_batch_info reports the call; refined: forward plus adjoint columns). With
 * U / D the launches of the node forest's up / down pass (nx_cp_batch_solve), the factor stage
 * is F = 1 + U and one solve pass without rhs and gather -- forward, up, down, back, residual,
 * norms -- is P = 4 + U + D. Steady, nothing refined:
 *   kind 1   per chunk  1 (rhs) + P + 1 (k_b_obs) + P + 1 (k_cp_b_edge_form)
 *   kind 0   per call   F + 1 (k_b_obs) + P;  per chunk  1 + P + 1 + 1
 *   kind 1   per call   F
 * A refinement pass adds P; a flushed assembly adds 1. A graph with cycles
 * (nx_set_cp_batch_cycles): P = 8 + 3 (U + D), and the call that builds the inverse adds
 * nx_cp_batch_solve's build launches.
 */
int nx_cp_batch_gradient(nx_network_t* h, int32_t n_cols, const double* edge_bc,
                         const double* edge_f, const double* f_const, double rtol, int32_t maxit,
                         int32_t kind, int32_t n_obs, const int32_t* obs_rows, const double* obs_w,
                         const double* obs_d, double* value, double* grad_R, double* grad_bc,
                         double* grad_f, int32_t* iters, double* relres, int32_t* converged);

/*
 * Ensembles: many resistance fields in one batched pass -- scenario j solves A(R_j) x_j = b_j,
 * a matrix per column (the reference would loop compute_forms + assemble + solve,
 * assembly.py:165-262, 329-368). The batched sweeps see R through the lumped flux mass alone, so
 * the chunk's set-up kernel (k_e_setup, in place of the rhs kernel) writes every column's own
 * lumped mass beside its right-hand side, with the assembly's expressions, and the true
 * residual (k_e_res) walks the handle's CSR pattern and regenerates the R-dependent values --
 * the flux-flux entries of an edge -- per column from R_j; the +-1 couplings and the multiplier
 * rows are read from the assembled values. A column whose R_j is the resident R has
 * nx_batch_solve's bits.
 *
 * nx_ensemble_supported: *ok = 1 where nx_batch_supported says 1 on a forest (tree_exact, no
 * cycle correction set: that correction is per matrix, 2 n_cyc solves per column -- a handle
 * opts in with nx_set_ensemble_cycles, below); elsewhere the calls below return NX_ERR_STATE.
 *
 * nx_ensemble_solve: n_cols scenarios.
 *   edge_R    n_cols x E, finite and positive (as nx_set_coefficients' edge_R, per scenario)
 *   edge_bc / edge_f / f_const / rtol / order / out / iters / relres / converged
 *             as nx_batch_solve
 * A pending deferred assembly is flushed first; the matrix must have been assembled (for any
 * R: only its R-independent values are read). Nothing of the handle is written: its edge_R,
 * values, lumped mass (not formed either), rhs, x, tmp, published state and snapshots stay as
 * they were. Chunks as nx_batch_solve; a workspace that serves ensembles carries E (N + 1) + E
 * more doubles per column (allocated on the first ensemble call). Per column: solve, true
 * residual against its own matrix, one refinement pass over the list of columns above rtol.
 * A column still above rtol is NOT handed to the single-column path (that path solves the
 * handle's matrix): it is reported converged = 0, iterations = 2, and the caller decides.
 * b = 0 gives x = 0, relres = 0, converged = 1. A column's bits do not depend on the other
 * columns, its position, n_cols or the chunk size.
 * NX_ERR_ARG: n_cols < 1, NULL edge_R / edge_bc / out, an R that is not finite and positive.
 * Launches (nx_get_batch_info reports these calls too; fallback stays 0): 7 per chunk -- set-up,
 * up, top, down, residual, norms, gather -- and 6 more for a chunk with a refinement pass.
 *
 * nx_ensemble_gradient: nx_batch_gradient with scenario j evaluated at R_j (edge_R as above,
 * the other arguments and outputs as nx_batch_gradient). The forward and the adjoint solve of a
 * column both run against the column's matrix, so the adjoint is per column for both kinds
 * (kind 0 has no shared adjoint column here); the derivative formulas are taken at R = 1 and
 * are nx_batch_gradient's. grad_R == NULL is legal: the objective alone -- the forward solve
 * and the observation kernel, no adjoint, n_cols doubles copied to the host (grad_bc / grad_f
 * are then ignored and the adjoint halves of iters / relres / converged left as they were).
 * Launches per chunk with S = 5: 1 + S + 1 + S + 1 = 13 (both kinds), 1 + S + 1 = 7 for the
 * objective alone, 6 more for each refinement pass.
 *
 * Graphs with cycles (nx_set_ensemble_cycles; off by default). The handle's cycle correction
 * (nx_set_cycles: Z = A_g^{-1} U and Cinv) belongs to the resident R, so the reference's one LU
 * per matrix (solver.py:58-65, after compute_forms + assemble, assembly.py:165-262, 329-368)
 * becomes a correction per scenario in the solve-again form, with m = 2 n_cyc, U the unit
 * columns of the cycle chains' rows and C the +-1 couplings the tree solve drops (they do not
 * depend on R):
 *   K_j = C^{-1} + U^T A_g(R_j)^{-1} U      (m x m, symmetric, indefinite)
 *   x_g = A_g(R_j)^{-1} b,  w = K_j^{-1} U^T x_g,  x = A_g(R_j)^{-1} (b - U w)
 * Z_j is never stored: per chunk of nc scenarios, right after the set-up kernel, the nc m unit
 * right-hand sides go through the batched sweeps in passes of as many columns as the workspace
 * holds (64 on such a handle, even for fewer scenarios; a pass may straddle scenarios, each
 * column with its scenario's lumped mass), only the rows of U are kept as K_j, and one workgroup
 * per scenario factorises K_j in place (LU, partial pivoting; in LDS while m^2 + m doubles fit a
 * workgroup's 160 KiB less 1 KiB, m <= 142, else in global memory -- the same operations, the
 * same bits). Every solve of the chunk -- 1 / 2 / 4 for nx_ensemble_solve / _gradient / _hvp,
 * refinement passes included -- then runs sweeps, k_e_cyc_w (w, and b - U w patched into the m
 * entries of the input column), sweeps, k_e_cyc_restore (the m entries put back bit for bit).
 * The results agree with nx_batch_solve at the same R to rounding, not bit for bit: the
 * solve-again form is a different sum from Z w. A zero coupling or a zero / non-finite pivot
 * flags the scenario: its columns get no correction, hold finite values and are reported
 * converged = 0. The workspace of a handle that has opted in carries m^2 + 2 m + 2 more
 * doubles per column behind everything else. Nothing of the handle is read but its pattern,
 * +-1 values and decomposition, and nothing written: no lumped mass, no cycle correction of
 * the handle's is built.
 *
 * nx_set_ensemble_cycles: handle state, enable = 0 / 1 (NX_ERR_ARG otherwise, and for a NULL
 * handle); it survives nx_set_preconditioner and nx_set_cycles. With 1, nx_ensemble_supported
 * also says 1 where nx_batch_supported does on a handle with 0 < n_cyc <= 512.
 * nx_get_ensemble_cycles: the flag, the last ensemble call's unit solves (n_cols m) and the
 * factor kernel's storage in its last chunk (0 none, 1 LDS, 2 global memory; NXHIP_ENS_CYC_LDS=0,
 * read per call, forces 2: a test hook). Any output may be NULL.
 *
 * Launches with cycles (nx_get_batch_info). With T the tree solve's launches (3: up, top, down;
 * 1 on a decomposition without jobs), W the workspace's columns (64 unless memory is short) and
 * per chunk of nc scenarios P = ceil(nc m / W):
 *   build per chunk   P (1 (k_e_cyc_unit) + T + 1 (k_e_cyc_extract)) + 1 (k_e_cyc_factor) = 5 P + 1
 *   per solve         T + 1 (k_e_cyc_w) + T + 1 (k_e_cyc_restore) + 2 (residual, norms): S = 10
 *   per refinement    S + 1 (update) = 11 in the chunk that has one
 * so nx_ensemble_solve takes 1 + (5 P + 1) + 10 + 1 (gather) = 5 P + 13 per chunk,
 * nx_ensemble_gradient 1 + (5 P + 1) + 2 S + 2 = 5 P + 24 (5 P + 13 for the objective alone), and
 * nx_ensemble_hvp 4 S + 7 + (5 P + 1) = 5 P + 48 (3 S + 6 + 5 P + 1 = 5 P + 37 with gauss_newton).
 *
 * nx_stash_solution: for a caller that loops nx_set_coefficients / nx_assemble / nx_solve over
 * scenarios on a handle that cannot take the calls above, and wants the handle back as it was.
 * restore = 0 saves x, tmp, the rhs and the published state of the last solve (a pending
 * deferred assembly is flushed first) into a buffer of the handle's (3 n_col doubles, allocated
 * on first use, freed by nx_destroy); restore = 1 puts them back, after flushing the assembly
 * of the coefficients the caller has put back, and forgets them (NX_ERR_STATE if nothing is
 * saved). The coefficients and the matrix values are the caller's to put back.
 */
int nx_ensemble_supported(nx_network_t* h, int32_t* ok);
int nx_ensemble_solve(nx_network_t* h, int32_t n_cols, const double* edge_R,
                      const double* edge_bc, const double* edge_f, const double* f_const,
                      double rtol, int32_t order, double* out, int32_t* iters, double* relres,
                      int32_t* converged);
int nx_ensemble_gradient(nx_network_t* h, int32_t n_cols, const double* edge_R,
                         const double* edge_bc, const double* edge_f, const double* f_const,
                         double rtol, int32_t kind, int32_t n_obs, const int32_t* obs_rows,
                         const double* obs_w, const double* obs_d, double* value, double* grad_R,
                         double* grad_bc, double* grad_f, int32_t* iters, double* relres,
                         int32_t* converged);
int nx_stash_solution(nx_network_t* h, int32_t restore);
int nx_set_ensemble_cycles(nx_network_t* h, int32_t enable);
int nx_get_ensemble_cycles(nx_network_t* h, int32_t* enabled, int32_t* unit_solves,
                           int32_t* storage);

/*
 * Hessian-vector products of nx_batch_gradient's objective: per scenario j the product H_j v_j
 * of the objective's Hessian with respect to (R, edge_bc, f) with a direction v_j = (dir_R,
 * dir_bc, dir_f), exact, in four batched direct solves (the reference has no counterpart). A is
 * affine in R, b linear in (edge_bc, f) and the device matrix symmetric, so with
 *   Ad = sum_e dir_R[e] dA/dR_e   (dir_R[e] times the R = 1 P1 mass on edge e's flux rows)
 *   bd = the right-hand side nx_batch_rhs forms from (dir_bc, dir_f)
 * the solves are: forward A x = b and adjoint A mu = c(x) (nx_batch_gradient's), the tangent
 * A xd = bd - Ad x, and the second-order adjoint A mud = cd - Ad mu with cd = w_i xd[r_i] on the
 * observed rows (kind 1) or 0 (kind 0). With form(l, x)[e] the cell sum of grad_R above:
 *   hess_R[j, e]     = -(form(mud, x)[e] + form(mu, xd)[e])
 *   hess_bc[j, e, .] = mud at the edge's q_0 / q_N row
 *   hess_f[j, e]     = -sum_k h_k mud[p_k]
 * and grad_R / grad_bc / grad_f (each may be NULL) are nx_batch_gradient's, bit for bit, from
 * the same pass. gauss_newton = 1 (kind 1 only): the second-order adjoint is A mud = cd and
 * hess_R = -form(mud, x) -- the product with J^T W J of the observed values' Jacobian, positive
 * semidefinite; no adjoint mu is solved (three solves), grad_* are ignored.
 *   dir_R   n_cols x E or NULL;  dir_bc  n_cols x E x 2 or NULL;  dir_f  n_cols x E or NULL
 *           (a NULL part is zero -- never the handle's source; any sign is legal)
 *   value   n_cols;  hess_R  n_cols x E;  hess_bc  n_cols x E x 2 or NULL;  hess_f  n_cols x E
 *           or NULL;  the other arguments as nx_batch_gradient
 *   iters / relres / converged  4 x n_cols each or NULL: forward, adjoint, tangent, second-order
 *           adjoint columns (gauss_newton: the adjoint quarter is left as it was; kind 0: its
 *           one adjoint column's figures for every scenario)
 * Every solve takes nx_batch_solve's per-column policy (residual check, refinement pass,
 * single-column fallback); a zero right-hand side gives an exact zero, converged. Supported
 * where nx_batch_supported says 1, else NX_ERR_STATE; the handle is left as nx_batch_gradient
 * leaves it. The workspace of a handle that has asked grows by two more vectors and 5 E doubles
 * per column (tangent, second-order adjoint; dir_R, hess_R, hess_f, hess_bc), behind everything
 * the earlier calls use; dir_bc / dir_f pass through the forward inputs' buffers. A column's
 * bits do not depend on the other columns, its position, n_cols or the chunk size.
 * NX_ERR_ARG: nx_batch_gradient's cases (hess_R in grad_R's place), all three of dir_R / dir_bc /
 * dir_f NULL, gauss_newton not 0 / 1, gauss_newton with kind 0.
 *
 * nx_get_batch_info then reports this call (refined: the columns of all four solves). Steady
 * launches when nothing is refined, S = 5 on a forest and 7 with cycles as above; the count
 * does not depend on n_cols inside a chunk nor on which direction parts are NULL:
 *   kind 1            per chunk  1 (rhs) + S + 1 (k_b_obs) + S + 1 (rhs of the direction)
 *                                + 1 (k_b_mass_apply) + S + 1 (k_b_obs_dir) + 1 (k_b_mass_apply)
 *                                + S + 1 (k_b_edge_form2) = 4 S + 7: 27 / 35
 *   kind 0            per call   1 (k_b_obs) + S: 6 / 8;  per chunk  3 S + 7: 22 / 28
 *   gauss_newton      per chunk  3 S + 6: 21 / 27   (no adjoint solve, one k_b_mass_apply)
 * and 6 / 8 more for each refinement pass.
 *
 * nx_ensemble_hvp: the same with scenario j evaluated at R_j (edge_R as nx_ensemble_solve): all
 * four solves of a column run against the column's matrix, dA/dR_e does not depend on R, the
 * adjoint is per column for both kinds. No single-column fallback: a column still above rtol
 * is reported converged = 0 in its quarter. Supported where nx_ensemble_supported says 1.
 * Launches per chunk with S = 5: 4 S + 7 = 27 (both kinds), 3 S + 6 = 21 with gauss_newton.
 */
int nx_batch_hvp(nx_network_t* h, int32_t n_cols, const double* edge_bc, const double* edge_f,
                 const double* f_const, double rtol, int32_t kind, int32_t n_obs,
                 const int32_t* obs_rows, const double* obs_w, const double* obs_d,
                 const double* dir_R, const double* dir_bc, const double* dir_f,
                 int32_t gauss_newton, double* value, double* grad_R, double* grad_bc,
                 double* grad_f, double* hess_R, double* hess_bc, double* hess_f, int32_t* iters,
                 double* relres, int32_t* converged);
int nx_ensemble_hvp(nx_network_t* h, int32_t n_cols, const double* edge_R, const double* edge_bc,
                    const double* edge_f, const double* f_const, double rtol, int32_t kind,
                    int32_t n_obs, const int32_t* obs_rows, const double* obs_w,
                    const double* obs_d, const double* dir_R, const double* dir_bc,
                    const double* dir_f, int32_t gauss_newton, double* value, double* grad_R,
                    double* grad_bc, double* grad_f, double* hess_R, double* hess_bc,
                    double* hess_f, int32_t* iters, double* relres, int32_t* converged);

/* Copy the owned part of the solution / rhs to the host (n_rows doubles). */
int nx_get_solution(nx_network_t* h, double* x);
int nx_get_rhs(nx_network_t* h, double* b);

/* The solution in the reference's function order -- what Solver.solve assigns into
 * [flux_color_0 .. flux_color_{M-1}, pressure, global_flux] (solver.py:120-134,
 * dolfinx.fem.petsc.assign). nx_set_output_map uploads once the permutation `rows`
 * (n_rows entries, a permutation of the owned rows: output position -> device row);
 * nx_get_solution_blocks gathers x into that order on the device and copies it to `out`
 * (n_rows doubles; pinned memory from nx_host_alloc makes the copy one DMA at PCIe
 * speed). Synchronous: `out` is complete when it returns. */
int nx_set_output_map(nx_network_t* h, int64_t n, const int32_t* rows);
int nx_get_solution_blocks(nx_network_t* h, double* out);

/* Deferred form of nx_get_solution_blocks (what Solver.solve returns by default):
 * nx_snapshot_solution gathers x into the function order into the handle's device
 * snapshot `slot` (0 <= slot < 64, allocated on first use) on the handle's stream and
 * returns without waiting -- later solves do not disturb it; nx_fetch_snapshot copies a
 * slot to `out` (n_rows doubles) on a separate copy stream once the gather has run and
 * waits for that copy only. The caller owns the slot bookkeeping (a slot is rewritten by
 * the next nx_snapshot_solution into it). Replaces the same assign as above
 * (solver.py:120-134): the functions' host arrays are filled when first read. */
int nx_snapshot_solution(nx_network_t* h, int32_t slot);
int nx_fetch_snapshot(nx_network_t* h, int32_t slot, double* out);

/* Page-locked host memory for nx_get_solution_blocks (hipHostMalloc / hipHostFree). */
int nx_host_alloc(int64_t bytes, void** out);
int nx_host_free(void* p);

/* Owned part of an internal vector (n_rows doubles): 0 = solution, 1 = rhs,
 * 2 = the latest preconditioned residual z = P^{-1} r (with the preconditioner). */
int nx_get_vector(nx_network_t* h, int32_t which, double* out);

/* Copy the assembled CSR (n_rows+1, nnz, nnz) to the host -- parity tests. */
int nx_get_csr(nx_network_t* h, int32_t* rowptr, int32_t* col, double* val);

/* y = A x for host vectors (x has n_cols entries incl. ghosts) -- tests. */
int nx_spmv_host(nx_network_t* h, const double* x, double* y);

/* True residual ||b - A x|| / ||b|| of the current device solution. */
int nx_true_residual(nx_network_t* h, double* relres);

/* Wait for all work queued on the handle's stream. */
int nx_sync(nx_network_t* h);

/*
 * Kernel timing with HIP events on the handle's stream.
 *   nx_set_profiling(h, 1) brackets every SpMV launch inside nx_solve with an
 *   event pair; nx_get_profile returns the summed SpMV time (ms), the number of
 *   timed SpMV launches, and the summed assembly kernel time (ms).
 *   nx_bench_spmv times `reps` back-to-back plain SpMV launches (ms per launch).
 */
int nx_set_profiling(nx_network_t* h, int32_t enable);
int nx_get_profile(nx_network_t* h, double* spmv_ms, int64_t* spmv_count, double* asm_ms,
                   int64_t* asm_count);
/* Direct solve (nx_set_solver 1, profiling on): summed kernel times (ms) of the up, top and
 * down sweeps (mode kModeDirect) and of the residual SpMV, over `count` direct solves, each
 * from events bound to the kernel's own dispatch (no graph while profiling). */
int nx_get_profile_direct(nx_network_t* h, double* ms4, int64_t* count);
/* How the direct solve checks its residual: *fused = 1 when the down sweep forms r = b - A x
 * itself (one rank, LDS kernels; the 4th time of nx_get_profile_direct is then the publish
 * kernel k_dir_publish_fr, which also forms the *n_left multiplier rows of the top part from
 * the CSR), 0 when a separate CSR SpMV (k_residual_ck) does. */
int nx_get_direct_info(nx_network_t* h, int32_t* fused, int32_t* n_left);
/* What the last direct solve ran: *path = 1 for the fused step k_dir_step (one rank, the
 * deferred assembly + the whole tree solve + the residual check + the published state in
 * one launch; under profiling its time is the 1st of nx_get_profile_direct, the others 0),
 * 0 for the separate launches (assembly, up sweep, down sweep, publish). Replaces nothing
 * in the reference (PETSc's KSPSolve is one call: solver.py:127). */
int nx_get_direct_path(nx_network_t* h, int32_t* path);
/* Whether the last fused or exchange step (path 1 or 3) ran phase 2 by superposition
 * (*sup = 1: the instantiation k_dir_step / k_dir_xr <W, CPL, true>, NXHIP_DIR_SUP; 0: the
 * plain phase 2). Replaces nothing in the reference (its profiling names). */
int nx_get_direct_sup(nx_network_t* h, int32_t* sup);
/* The dense top of the fused step (one rank, superposition, the dense lists of
 * nx_set_pc_dense; NXHIP_DIR_DENSE=0 switches it off per solve): *ran = 1 when the last
 * k_dir_step formed its top values as rows of G times the posted inputs instead of solving
 * the top part in one workgroup; *builds = how many times this handle has built G (once per
 * decomposition and per contents of R: new boundary values or a new source do not rebuild
 * it). Either pointer may be NULL. Replaces nothing in the reference. */
int nx_get_direct_dense(nx_network_t* h, int32_t* ran, int32_t* builds);
/* The CSR values kept across assemblies while R is unchanged (one rank, P1/DG0; DESIGN.md
 * section 3c, round 8): the values depend on the geometry, N and R alone, so once a launch has
 * written all of them for the resident R, later assemblies and fused steps store only the rhs
 * (NXHIP_KEEP_VALUES=0, read per solve, makes every one store them). *last_step_kept = 1 when
 * the last assembly launch or fused step that was asked for the matrix left the values in
 * device memory alone; *value_writes = how many launches of this handle have written them.
 * R set to new contents -- changed and changed back included -- is written again once.
 * Either pointer may be NULL. Replaces the caller-side choice between the reference's
 * assemble_lhs and assemble_rhs (assembly.py:333-358, solver.py:101). */
int nx_get_values_kept(nx_network_t* h, int32_t* last_step_kept, int64_t* value_writes);
/* The chains' R-only factors kept across values-free steps:
 * every cell's length h and mass R h / 6 and every chain's T, 1 / T, mo and 1 / mo depend on
 * the geometry, N, the decomposition and R alone, so the values-free dense step reads them
 * from a per-handle table (k_dir_step_kg) instead of forming them in every launch. The table
 * is built by the step's own device functions (the same bits), lazily before the first such
 * step, and again only after R's contents or the decomposition changed; new boundary values
 * or a new source leave it alone (NXHIP_KEEP_GEO=0, read per solve, keeps the recomputing
 * step k_dir_step_kv). *ran = 1 when the last step read the table; *builds = how many times
 * this handle built it. Either pointer may be NULL. Replaces nothing in the reference. */
int nx_get_geo_kept(nx_network_t* h, int32_t* ran, int32_t* builds);
/* (path 2: the (k, 0) condensed route of nx_fe_set_direct; path 4: the continuous-pressure
 * node-condensed route of nx_fe_set_cp; path 3: several ranks, the
 * exchange step k_dir_xr / k_dir_xg, one launch per rank.)
 * Test hook: the number of s_sleep-paced polls a k_dir_step workgroup spends waiting for the
 * top part's values before it gives up (default 2^20). 0 makes every waiting workgroup give
 * up at once, which forces the fallback a non-co-resident launch takes: the host resets the
 * hand-off counters and the device's published-state count and runs the separate launches
 * on this handle from then on (until the next nx_set_preconditioner). Replaces nothing in
 * the reference. */
int nx_debug_set_wait_polls(nx_network_t* h, uint32_t polls);
/* Test hook: the kernels' segment cross-lane helpers (seg_up / seg_down / seg_xor, their _nc
 * variants, seg_bcast0, seg_incl_scan, seg_sum, wave_sum: DPP row moves for segments of 4, 8
 * and 16 lanes) beside the plain __shfl* they replace, on the same input, in one launch of
 * one 1024-thread workgroup on the current device. in_d / in_i: 1024 values, one per lane.
 * Outputs: *n_slots slots of 1024 values each (cap_slots: what the four arrays hold; 64 is
 * enough), new_* by the helpers and ref_* by the shuffles. Slots, for W = 4, 8, 16 in turn:
 * for O = 1, 2, .. < W the moves up, down, xor, up_nc, down_nc; then bcast0, inclusive scan,
 * sum; the last slot is wave_sum. The three sums are zero in the int outputs. Replaces nothing
 * in the reference. */
int nx_test_seg_shuffle(const double* in_d, const int32_t* in_i, int32_t cap_slots,
                        double* new_d, double* ref_d, int32_t* new_i, int32_t* ref_i,
                        int32_t* n_slots);
/* Rehearsal hook: the exchange step (k_dir_xr) of group member h ALONE, reps timed launches
 * (*ms: average kernel time, HIP events on the dispatch), its two exchanges emulated from
 * the sums the group's previous graph-path direct solve left -- the per-rank time of a
 * multi-GPU run measured on one GPU (whose ranks cannot all be resident in one launch).
 * h's solution is then the rank's share of the answer. Replaces nothing in the reference. */
int nx_debug_xr_rehearse(nx_network_t* h, double rtol, int32_t reps, double* ms);

/* Debug / tests: the RCCL ranks' shape of the exchange step on one GPU -- every rank of the
 * group launches its own k_dir_xr on a stream of its own (concurrent launches meeting only
 * through the mailboxes, the exchange width the handle's rank count), the ranks' assembly
 * pending. *relres = the published residual (every rank's equal). */
int nx_debug_xr_separate(nx_group_t* g, double rtol, double* relres);
/* A rank that gives up an exchange raises an abort word in every rank's mailbox, so the
 * other ranks' exchanges fail at once; the ranks then agree, through one max-all-reduce of
 * four doubles, on who finished which step, so every rank leaves the exchange step at the
 * same point and no collective of the graph path is ever paired across steps (the rank that
 * gave up exchange 2 of a step the others finished keeps its final x and takes their
 * published residual). Test hook: the poll bound of this rank's exchange `which` (0: the
 * coarse partials, 1: the residual) in its next steps; 0 makes it give up at once, after
 * its own slots and flags are written. Replaces nothing in the reference. */
int nx_debug_xr_polls(nx_network_t* h, int32_t which, uint32_t polls);
/* out[4] = [the exchange step is off for good (agreed), the last launch's give-up reasons
 * (bits: 1 exchange 1, 2 exchange 2, 4 another rank's abort seen, 8 a slot with another
 * launch's tag, 16 a local wait), agreements this rank took part in, the last launch's tag]. */
int nx_get_xr_status(nx_network_t* h, int32_t* out);
int nx_reset_profile(nx_network_t* h);
int nx_bench_spmv(nx_network_t* h, int32_t reps, double* ms_per_spmv);
/* The same SpMV rotating over private copies of the CSR and vectors (> 512 MiB in total,
 * twice the Infinity Cache) so every launch streams from HBM ("cold"). */
int nx_bench_spmv_cold(nx_network_t* h, int32_t reps, int32_t* copies, double* ms_per_spmv);

/*
 * Multi-GPU (one process per GPU). Rank 0 creates the RCCL unique id, the
 * host control plane (torch.distributed) broadcasts it, every rank calls
 * nx_comm_init with its halo plan. Replaces the MPI ghost updates
 * (assembly.py:363-367, solver.py:128-132) and MUMPS' internal communication.
 *   n_peers                 neighbouring ranks
 *   peer_rank[n_peers]
 *   send_off[n_peers+1], send_idx[...]   owned local rows to send to each peer
 *   recv_off[n_peers+1]     ghost slots [recv_off[p], recv_off[p+1]) filled by peer p
 * nx_set_halo records the plan only; nx_comm_init = nx_set_halo + the RCCL communicator.
 * Both must precede nx_set_preconditioner.
 */
int nx_comm_unique_id(unsigned char* id_out /* NX_UNIQUE_ID_BYTES */);
int nx_set_halo(nx_network_t* h, int32_t nranks, int32_t rank, int32_t n_peers,
                const int32_t* peer_rank, const int32_t* send_off, const int32_t* send_idx,
                const int32_t* recv_off);
int nx_comm_init(nx_network_t* h, int32_t nranks, int32_t rank, const unsigned char* id,
                 int32_t n_peers, const int32_t* peer_rank, const int32_t* send_off,
                 const int32_t* send_idx, const int32_t* recv_off);
/* Tests: nx_comm_init with a host transport in place of RCCL -- several ranks' processes on
 * ONE GPU (RCCL refuses two ranks on one device), collectives through the POSIX shared
 * memory `name` ("/..."; the same on every rank, chosen by rank 0 and broadcast), eager
 * (every collective synchronises the stream; no graph capture). It runs the RCCL ranks' host
 * logic unchanged: the exchange step over IPC-mapped mailboxes, its agreement, the graph
 * path. Not a performance path. Replaces nothing in the reference. */
int nx_comm_init_host(nx_network_t* h, int32_t nranks, int32_t rank, const char* name,
                      int32_t n_peers, const int32_t* peer_rank, const int32_t* send_off,
                      const int32_t* send_idx, const int32_t* recv_off);

/* Several ranks, direct solve: the multiplier rows of the K cut bifurcations (incident
 * edges on several ranks; one global order, the same on every rank) are completed inside
 * the residual's all-reduce of [||r||^2, ||b||^2, r_cut[K]] instead of a halo of x and a
 * second all-reduce -- the MPI ghost update + norm of the reference's solve
 * (solver.py:128-132, assembly.py:363-367) in one collective.
 *   lm_cut[n_lm]        per owned multiplier row (local order): its cut index or -1
 *   gk_off[K+1], gk_row, gk_coef   per cut index owned by another rank: this rank's flux
 *                       end rows at it and their coupling coefficient (+-1)
 * NXHIP_DIR_CUT=0 keeps the halo path. Part of the ranks' schedule signature. */
int nx_set_cut(nx_network_t* h, int32_t K, const int32_t* lm_cut, const int32_t* gk_off,
               const int32_t* gk_row, const double* gk_coef);

/* Several ranks, direct solve in ONE launch per rank (k_dir_xr): the ranks exchange the
 * coarse partials and the residual's partials device-side, through a mailbox in each rank's
 * device memory that every rank writes into (IPC-mapped over xGMI) -- no RCCL call in the
 * step. After nx_comm_init: nx_xch_export writes this rank's mailbox handle
 * (NX_XCH_HANDLE_BYTES); the host control plane all-gathers them in rank order; every
 * rank passes all P to nx_xch_import. The ranks decide together (the schedule comparison)
 * whether every one can run the step; otherwise the graph path (RCCL all-reduces) runs.
 * NXHIP_DIR_XR=0 keeps the graph path. Replaces the MPI reductions of the reference's
 * distributed MUMPS solve (solver.py:127-132); in-process groups link their mailboxes in
 * nx_group_create. */
#define NX_XCH_HANDLE_BYTES 64
int nx_xch_export(nx_network_t* h, unsigned char* handle_out);
int nx_xch_import(nx_network_t* h, const unsigned char* handles);

/* Ranks of the handle's RCCL communicator (ncclCommCount); without one, the rank count of
 * its halo plan (1 for a single-GPU handle). bench.py reports it next to the timing. */
int nx_comm_count(nx_network_t* h, int32_t* nranks);

/*
 * In-process rank group: the ranks of a partitioned problem as handles on ONE device,
 * driven in lock-step from one host thread, with the halo exchange as device copies and
 * the all-reduces as a fixed-order device sum. Same kernels and schedule as the RCCL path,
 * so a multi-rank solve can be checked on a single GPU (RCCL rejects two ranks on one
 * device). Each handle h_r needs nx_set_halo(h_r, nranks, r, ...) first; the group lends
 * the handles one shared stream until nx_group_destroy (which must precede nx_destroy).
 * nx_group_solve = nx_solve over all ranks; fails with NX_ERR_STATE if the ranks' MINRES
 * recurrences ever differ.
 */
int nx_group_create(int32_t nranks, nx_network_t* const* handles, nx_group_t** out);
int nx_group_solve(nx_group_t* g, double rtol, int32_t maxit, int32_t check_every,
                   int32_t* iters, double* relres, int32_t* converged);
int nx_group_destroy(nx_group_t* g);

#ifdef __cplusplus
}
#endif

#endif /* NXHIP_H */
