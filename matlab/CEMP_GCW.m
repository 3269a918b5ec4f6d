%% CEMP_GCW -- drop-in replacement of the reference's Algorithms/CEMP_GCW.m (CEMP, then the spectral step weighted by 1/(SVec + 1e-8))
function R_est = CEMP_GCW(Ind, RijMat, CEMP_parameters)
    [IndS, perm] = sortrows(double(Ind), [1 2]);
    seed = 0; if isfield(CEMP_parameters, 'seed'), seed = CEMP_parameters.seed; end
    R_est = desc_amd_mex('cemp_gcw', int32(IndS - 1), double(RijMat(:,:,perm)), double(CEMP_parameters.reweighting(:)'), ...
                         CEMP_parameters.max_iter, CEMP_parameters.nsample, seed);
end
