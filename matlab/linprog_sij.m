%% linprog_sij -- drop-in replacement of the reference's Algorithms/linprog_sij.m:16:   [Rest, S_vec] = linprog_sij(Ind, RijMat)
%% The LP  min sum s_ij  s.t.  |s_ij - d_ijk| <= s_ik + s_jk  on sampled 3-cycles, 0 <= s <= 1 (:16-139; MATLAB's linprog is replaced by a
%% matrix-free PDHG solver on the MI355X), the spectral step weighted by exp(-5 S_vec) (:154-174) and the reweighted Lie-algebraic
%% refinement with maxIters = 200 (:176-351), on one device problem.  Optional third argument, not in the reference: a struct with any of
%% seed, device, tol (1e-4), max_iter (200000), nsample (0: the rule of :43), verbose.  Third output: the LP's record.
function [Rest, S_vec, info] = linprog_sij(Ind, RijMat, opt)
    if nargin < 3, opt = struct(); end
    [IndS, perm] = sortrows(double(Ind), [1 2]);
    [Rest, S_sorted, info] = desc_amd_mex('lp', int32(IndS - 1), double(RijMat(:,:,perm)), opt);
    for l = 1000:1000:info.m_pos, disp('next 1000 done'); end      % linprog_sij.m:115-117
    S_vec = ones(1, size(Ind,1));                                  % :104
    S_vec(perm) = S_sorted;
end
