%% IRLS_GM -- drop-in replacement of the reference's Algorithms/IRLS_GM.m (L1 initialisation + Geman-McClure IRLS, on the GPU).
% R = IRLS_GM(RijMat, Ind, 'Rinit', Rinit, 'SIGMA', 5, 'MaxIterations', [10 100]); RijMat comes first, as in the reference.
% Nodes outside the largest connected component get NaN.
function R = IRLS_GM(RijMat, Ind, varargin)
    R = irls_call('irls_gm', RijMat, Ind, varargin{:});
end

function R = irls_call(cmd, RijMat, Ind, varargin)
    inp = inputParser;
    inp.addParameter('Rinit', []);
    inp.addParameter('SIGMA', 5);
    inp.addParameter('MaxIterations', [10 100]);
    inp.parse(varargin{:});
    a = inp.Results;
    if ndims(RijMat) ~= 3 || size(RijMat, 1) ~= 3, error('IRLS_GM: RijMat must be 3 x 3 x m (the quaternion form is not supported)'); end
    if isempty(a.SIGMA), a.SIGMA = 5; end
    [IndS, perm] = sortrows(double(Ind), [1 2]);
    order0 = zeros(numel(perm), 1, 'int32'); order0(:) = int32(perm - 1);
    R = desc_amd_mex(cmd, int32(IndS - 1), double(RijMat(:,:,perm)), order0, a.MaxIterations(1), a.MaxIterations(2), ...
                     a.SIGMA, double(a.Rinit));
end
