%% DESC_init -- drop-in replacement of the reference's Algorithms/DESC_init.m:14:   [R_est, S_vec] = DESC_init(Ind, RijMat, params)
%% DESC_PGD (DESC_init.m:16-253) followed by GCW (:255), without the refinement: what DESC() returns as R_init and S_vec.  The reference
%% appends MSE_means and svec_errors to two CSV files in the current directory whenever it plots (:262-263); here that happens only when
%% params.csv_dir names a directory.
function [R_est, S_vec] = DESC_init(Ind, RijMat, params)
    make_plots = isfield(params, 'make_plots') && params.make_plots;
    if make_plots
        [S_vec, traces] = DESC_PGD(Ind, RijMat, params);
    else
        S_vec = DESC_PGD(Ind, RijMat, params);
    end
    [IndS, perm] = sortrows(double(Ind), [1 2]);
    R_est = desc_amd_mex('gcw', int32(IndS - 1), double(RijMat(:,:,perm)), S_vec(perm));          % :255
    if make_plots
        if isfield(params, 'csv_dir')                                                             % :262-263
            dlmwrite(fullfile(params.csv_dir, 'linear_convergence_rotation_error.csv'), traces.MSE_means, 'delimiter', ',', '-append');
            dlmwrite(fullfile(params.csv_dir, 'linear_convergence_svec_error.csv'), traces.svec_errors, 'delimiter', ',', '-append');
        end
        names = {'svec_errors', 'obj_vals', 'MSE_means', 'MSE_medians'};                          % the 2 x 2 figure of :258-290
        labels = {'Average distance to true corruption', 'Value of Objective Function', ...
                  'Mean Error in R estimate (degrees)', 'Median Error in R estimate (degrees)'};
        figure;
        for q = 1:4
            subplot(2, 2, q); plot(1:numel(traces.(names{q})), traces.(names{q}));
            xlabel('Iteration number'); ylabel(labels{q});
        end
    end
end
