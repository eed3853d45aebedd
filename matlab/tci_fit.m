function [MCMCresults, MCMCplot, MCMCchain, MCMCdiag, MCMClp, MCMCstack, MCMCtemper, MCMCsearch, MCMCdemc, MCMCrank, MCMCdemczs] = tci_fit(data, varargin)
%TCI_FIT One dataset of TranscriptionCycleMCMC on an MI355X: every cell's DRAM chain in one launch.
%   [MCMCresults, MCMCplot, MCMCchain] = TCI_FIT(data, Name, Value, ...) replaces the body of the
%   parfor over cells of src/TranscriptionCycleMCMC.m:161-357 and the pruning of skipped cells
%   (:359-369) for ONE dataset. data is the dataset's struct array (fields time, MS2, PP7, name;
%   README.md:11-16), i.e. data_all(k).data at :146. The three outputs are the reference's structs
%   with the reference's fields, one element per fitted cell in cell order; save them as :371-378 do.
%
%   Where the reference runs one mcmcrun per cell in a parfor worker, with a MATLAB ssfun handle,
%   TCI_FIT sets every cell up exactly as :163-270 do, then makes ONE tci_mex('dram', ...) call:
%   mcmcstat's DRAM (proposals, bounds rejection, delayed rejection, covariance adaptation, the
%   Gaussian dR priors and the sigma^2 Gibbs update) for all cells at once on the GPU, every ssfun
%   evaluation a HIP kernel (matlab/tci_mex.cpp -> include/tci.h tci_dram_run). The summaries
%   (:276-303) come back reduced on the device; the forward model at the means (:307-309) is
%   tci_mex('forward', ..., 'raw').
%
%   Name-value options -- the reference's names and defaults (:36-45, :57-77):
%     'n_burn' (10000), 'n_steps' (20000), 'ratePriorWidth' (50), 't_start' (0), 't_end' (Inf),
%     'construct' ('P2P-MS2v5-LacZ-PP7v4', or a struct: see tci_mex 'create'),
%     'previous' ([]: no loadPrevious; else the MCMCresults struct array of an earlier fit -- the
%        hierarchical fit of :84-107, v fixed to previous mean_v +- 1e-5 (:193-198, :217-241),
%        ApprovedFits carried over (:345-347), cells without an entry skipped (:196-198))
%   and the GPU's own:
%     'device' (0), 'cells' (all: 1-based cell numbers to fit -- one GPU's share of a dataset),
%     'thin' (1 = every chain row, as the reference keeps them; k keeps rows 1, 1+k, ...; 0 keeps none
%        and MCMCchain is empty), 'seed' (0), 'engine' ('auto'), 'adapt_pmax' (0; see include/tci.h),
%     'predict' (0: none; nsample > 0 adds the predictive bands of mcmcstat's mcmcpred to MCMCplot:
%        predMS2 and predPP7 (3 x N: the 2.5 %, 50 % and 97.5 % quantiles, at every time point, of the
%        forward model at nsample posterior samples) and pred_probs, one tci_mex('predict', ...) call for
%        all cells. Needs 'thin' > 0. Where mcmcpred draws chain rows at random, the rows used here
%        are round(linspace(1, rows, nsample)) of the post-burn-in rows kept (all of them when fewer),
%        at most 4096.)
%     'diagnostics' (0; 1 fills the fourth output MCMCdiag, one entry per fitted cell: mcmcstat's
%        chainstats columns reduced on the device from the rows MCMCchain keeps -- mcerr_*, tau_* and
%        geweke_p_* for v, ton, A, tau, MS2_basal, PP7_basal, R, dR (vectors) and s2, n_rows,
%        ess_min = n_rows / max tau and cell_index; formulas in include/tci.h. Needs 'thin' > 0.)
%     'logpost' (0; 1 fills the fifth output MCMClp, one entry per fitted cell: the sum-of-squares trace ss
%        (mcmcstat's sschain, mcmcrun's fourth output) and the log-posterior trace lp of the rows MCMCchain
%        keeps, ss_min, ss_mean, dev_mean, dev_var, the best sample (best_row, 1-based among those rows, lp_best,
%        ss_best, s2_best and best_v, best_ton, .. best_dR), s2_mean, ss_hat, d_hat, p_d, p_v, dic, n_rows and
%        cell_index, all on the device (tci_mex('dram') options.logpost; formulas in include/tci.h). Needs
%        'thin' > 0.)
%     'stack' (0; nsample in [32, 4096] fills the sixth output MCMCstack, one entry per fitted cell: the PSIS-LOO
%        log predictive density elpd_loo_i and Pareto k khat_i of every observed value (2 x N, row 1 = MS2), elpd_loo,
%        p_loo, khat_max, n_khat_bad, the stacking weights (1 for the one chain a cell has here), elpd_stack,
%        n_samples and cell_index, over rows round(linspace(1, rows, nsample)) of the post-burn-in rows kept, on the
%        device (tci_mex('dram') options.stack; formulas in include/tci.h). Needs 'thin' > 0 and 32 such rows.)
%     'temper' (1; R > 1 runs a ladder of R chains per cell at inverse temperatures beta_r = q^r,
%        q = 1/(1 + sqrt(2/(7 + N))), whose neighbouring rungs exchange states after every 'swap_every'-th (1)
%        adaptation window on the device (parallel tempering: tci_mex('dram') options.temper; include/tci.h). Chain
%        column r*nc + k is rung r of fitted cell k: the cold rungs (beta = 1) come first and every other output is
%        theirs; a hot rung starts from its own draw of x0 and runs on RNG stream cellNum - 1 + r*2^24. Fills the
%        seventh output MCMCtemper, one entry per fitted cell: beta (1 x R), swap_rate and swap_tried (1 x R-1, per
%        pair of neighbouring rungs; NaN for a pair never tried), accept_rate (1 x R), swap_every, n_events, cell_index.
%        Not with 'logpost' or 'stack'.)
%     'presearch' ([]; [n_pop n_gen] runs a mode search before the chains start: differential evolution on
%        ss/sigma2 + prior over n_pop members per fitted cell for n_gen generations on the device
%        (tci_mex('modesearch'); include/tci.h). Member 1 of a cell is its usual x0, the others are drawn as x0
%        is; the search is seeded as the sampler is and keyed by cellNum - 1. The cell's chain, and with 'temper'
%        every rung of its ladder, starts from the best member. Fills the eighth output MCMCsearch, one entry per
%        fitted cell: f_best, ss_best, theta_best (1 x 7+N), f0_best (the best of the initial population), f_trace
%        (1 x n_gen+1), n_gen, n_pop, n_evals, cell_index.)
%     'demc' ([]; [n_pop n_gen] samples every fitted cell with the DE-MC population sampler instead of DRAM:
%        n_pop members per cell for n_gen generations on the device (tci_mex('demc'); include/tci.h). The members
%        start as 'presearch' draws them, or from the search's final population when 'presearch' is given with the
%        same n_pop; the jitter is 1e-3*sqrt(J0); the run is seeded as the sampler is and keyed by cellNum - 1.
%        n_burn counts generations and thin > 0 is needed; n_steps is not used. Every output comes from the kept
%        rows of generations >= n_burn of all members pooled (mean_sigma and sigma_sigma included; s2chain holds
%        every kept row). Fills the ninth output MCMCdemc, one entry per fitted cell: accept_rate, n_oob, n_evals
%        (1 x n_pop), rhat_max, ess_min (across the members, parameters and sigma2), n_pop, n_gen, cell_index.
%        Not with 'temper', 'diagnostics', 'logpost', 'stack' or 'predict'.)
%     'demczs' ([]; [n_pop n_gen] samples every fitted cell with the DE-MC(zs) sampler (tci_mex('demczs');
%        include/tci.h): n_pop chains per cell, 1 to 4096, that propose from an archive of past states. The archive
%        starts with m0 = min(10*P, 4096) rows, P the longest cell's 7+N, drawn as 'presearch' draws a population, and
%        the chains start at its first n_pop rows; with 'presearch' [m0 n_gen] the search's final population is the
%        archive and the chains start at its best members. Everything else is as for 'demc', whose place the chains
%        take. Fills the eleventh output MCMCdemczs: MCMCdemc's fields plus n_null (1 x n_pop), snooker_rate (the
%        share of snooker moves among the first min(n_gen, 1024) generations, the ones that are logged), m0 and
%        n_archive. Not with 'demc'.)
%     'bounds' ('reject'; with 'demczs': 'reflect' reflects a coordinate that leaves its box back into it, with an
%        orientation bit per coordinate, instead of rejecting the proposal (tci_demczs_run_bounds, include/tci.h);
%        MCMCdemczs gains reflect_rate, the evaluated proposals with a reflection over all proposals.)
%     'census' (0; with 'demczs': 1 counts, per coordinate, how often it crossed and how often it left below or
%        above its bound; MCMCdemczs gains n_cross, oob_lo, oob_hi (1 x 7+N, summed over the chains) and oob_share,
%        (oob_lo + oob_hi) over the cell's bounds-rejected proposals (NaN with 'reflect').)
%     'rank' (0; 1 fills the tenth output MCMCrank, one entry per fitted cell, with the rank diagnostics of Vehtari et
%        al. (2021) over the kept rows at or past n_burn (tci_chainrank, include/tci.h; options.rank of
%        tci_mex('dram') / tci_mex('demc'), reduced from the device chain): across the cell's DE-MC members with
%        'demc', else of the cell's one chain (its two halves). Fields, 7+N+1 columns wide (theta order, sigma2
%        last): q (nq x .) at probs, q_tail (2 x .) at tail, rhat_bulk, rhat_folded, rhat_rank, ess_bulk, tau_bulk,
%        ess_tail_lo, ess_tail_hi, ess_tail, window_bulk, window_tail_lo, window_tail_hi (1 x .), n_rows,
%        cell_index. Needs 'thin' > 0; not with 'temper' or 'logpost'.)
%
%   x0 is drawn from MATLAB's global RNG exactly as :200-208 draw it (rand, normrnd); the chains use
%   the device's Philox streams keyed by (seed, cell number), so a cell's chain does not depend on
%   which other cells are fitted with it or on which GPU. Sampling follows mcmcstat's published
%   algorithm, so a fit reproduces the reference's posterior, not MATLAB's random draws.
%
%   Spreading a dataset over the GPUs of a node (one MATLAB worker per GPU, e.g. spmd):
%       share = labindex:numlabs:numel(data);
%       [r, p, c] = tci_fit(data, 'cells', share, 'device', labindex - 1);
%   then concatenate the workers' outputs and sort them by cell_index.

p = inputParser;
p.addParameter('n_burn', 10000);
p.addParameter('n_steps', 20000);
p.addParameter('ratePriorWidth', 50);
p.addParameter('t_start', 0);
p.addParameter('t_end', Inf);
p.addParameter('construct', 'P2P-MS2v5-LacZ-PP7v4');
p.addParameter('previous', []);
p.addParameter('device', 0);
p.addParameter('cells', []);
p.addParameter('thin', 1);
p.addParameter('seed', 0);
p.addParameter('engine', 'auto');
p.addParameter('adapt_pmax', 0);
p.addParameter('predict', 0);
p.addParameter('diagnostics', 0);
p.addParameter('logpost', 0);
p.addParameter('stack', 0);
p.addParameter('temper', 1);
p.addParameter('swap_every', 1);
p.addParameter('presearch', []);
p.addParameter('demc', []);
p.addParameter('demczs', []);
p.addParameter('bounds', 'reject');
p.addParameter('census', 0);
p.addParameter('rank', 0);
p.parse(varargin{:});
o = p.Results;
n_burn = o.n_burn;
n_steps = o.n_steps;
loadPrevious = ~isempty(o.previous);
N = length(data);                                   % :146
cellNums = o.cells;
if isempty(cellNums)
    cellNums = 1:N;
end

% ---- per-cell setup, as the parfor body does it (:163-255) --------------------------------------
setup = struct('cellNum', {}, 't', {}, 'MS2', {}, 'PP7', {}, 'x0', {}, 'lb', {}, 'ub', {}, 'mu', {}, ...
    'sig', {}, 'J0', {}, 'approved', {});
for cellNum = cellNums(:)'
    t = data(cellNum).time;                         % :163-167
    MS2 = data(cellNum).MS2;
    PP7 = data(cellNum).PP7;
    indStart = find(t >= o.t_start, 1, 'first');    % :170-175
    indEnd = find(t < o.t_end, 1, 'last');
    t = t(indStart:indEnd);
    MS2 = MS2(indStart:indEnd);
    PP7 = PP7(indStart:indEnd);
    approved = 0;                                   % :349
    if loadPrevious                                 % :193-198
        cellToload = find([o.previous.cell_index] == cellNum, 1);
        if isempty(cellToload) || isempty(o.previous(cellToload).mean_v) || ...
                ~isfinite(o.previous(cellToload).mean_v)
            continue
        end
        v0 = o.previous(cellToload).mean_v;
        approved = o.previous(cellToload).ApprovedFits;   % :345-347
    else
        v0 = 1+2*rand;                              % :200
    end
    ton0 = 4*rand;                                  % :202-208
    A0 = rand;
    tau0 = 4*rand;
    MS2_basal0 = 10;
    PP7_basal0 = 5;
    R0 = 15;
    dR0 = normrnd(0,3,1,length(t));
    x0 = [v0,tau0,ton0,MS2_basal0,PP7_basal0,A0,R0,dR0];   % :210
    if loadPrevious                                 % :217-221
        v_step = 0.0000001;
        v_lower = v0-0.00001;                       % :235-241
        v_upper = v0+0.00001;
    else
        v_step = 0.05;
        v_lower = 0;
        v_upper = 10;
    end
    ton_step = t(end)-t(end-1);                     % :222-231: diag(J0)
    J0 = [v_step, 0.1, ton_step, 1, 1, 0.05, 0.5, 0.5*ones(size(dR0))];
    n = length(t);                                  % :242-255: params {name, x0, lower, upper, mu, sig}
    lb = [v_lower, 0, 0, 0, 0, 0, 0, -30*ones(1,n)];
    ub = [v_upper, 20, 10, 50, 50, 1, 40, 30*ones(1,n)];
    mu = zeros(1, 7+n);
    sig = [Inf(1,7), o.ratePriorWidth*ones(1,n)];
    setup(end+1) = struct('cellNum', cellNum, 't', t, 'MS2', MS2, 'PP7', PP7, 'x0', x0, 'lb', lb, ...
        'ub', ub, 'mu', mu, 'sig', sig, 'J0', J0, 'approved', approved); %#ok<AGROW>
end
MCMCresults = struct('mean_v',{},'sigma_v',{},'mean_ton',{},'sigma_ton',{},...   % :149-157
    'mean_A',{},'sigma_A',{},'mean_tau',{},'sigma_tau',{},...
    'mean_MS2_basal',{},'sigma_MS2_basal',{},'mean_PP7_basal',{},'sigma_PP7_basal',{},'mean_R',{},...
    'sigma_R',{},'mean_dR',{},'sigma_dR',{},'mean_sigma',{},'sigma_sigma',{},...
    'cell_index',{},'ApprovedFits',{});
if o.predict > 0
    if o.thin <= 0
        error('tci:predict', 'predict needs the chain rows: use thin > 0');
    end
    MCMCplot = struct('t_plot',{},'MS2_plot',{},'PP7_plot',{},'simMS2',{},'simPP7',{}, ...
        'predMS2',{},'predPP7',{},'pred_probs',{});
else
    MCMCplot = struct('t_plot',{},'MS2_plot',{},'PP7_plot',{},'simMS2',{},'simPP7',{});
end
MCMCchain = struct('v_chain',{},'ton_chain',{},'A_chain',{},'tau_chain',{},...
    'MS2_basal_chain',{},'PP7_basal_chain',{},'R_chain',{},'dR_chain',{},'s2chain',{});
MCMCdiag = struct([]); MCMClp = struct([]); MCMCstack = struct([]); MCMCtemper = struct([]);
MCMCsearch = struct([]); MCMCdemc = struct([]); MCMCrank = struct([]); MCMCdemczs = struct([]);
if o.rank && o.thin <= 0
    error('tci:rank', 'the rank diagnostics need the kept chain rows: thin > 0');
end
nc = numel(setup);
if nc == 0
    return
end

% ---- one context over the fitted cells, one column per chain (padding past a chain's 7 + N) -------
cellData = struct('time', {setup.t}, 'MS2', {setup.MS2}, 'PP7', {setup.PP7});
h = tci_mex('create', cellData, o.construct, o.device);
cleanup = onCleanup(@() tci_mex('destroy', h));
P = 7 + max(arrayfun(@(f) numel(f.t), setup));
X0 = zeros(P, nc); LB = -Inf(P, nc); UB = Inf(P, nc); MU = zeros(P, nc); SIG = Inf(P, nc); J0 = ones(P, nc);
for k = 1:nc
    m = numel(setup(k).x0);
    X0(1:m, k) = setup(k).x0;
    LB(1:m, k) = setup(k).lb;
    UB(1:m, k) = setup(k).ub;
    MU(1:m, k) = setup(k).mu;
    SIG(1:m, k) = setup(k).sig;
    J0(1:m, k) = setup(k).J0;
end
R = o.temper;
if ~(isscalar(R) && R >= 1 && R == floor(R) && R <= 256)
    error('tci:temper', 'temper must be an integer rung count in [1, 256]');
end
if R > 1 && (o.logpost || o.stack)
    error('tci:temper', 'temper > 1 cannot be combined with logpost or stack');
end
keys = [setup.cellNum] - 1;
cols = 1:nc;
if R > 1                                            % the hot rungs: columns r*nc + k, their own x0
    temper = [ones(1, nc*R); repmat(1:nc, 1, R)];
    for r = 1:R-1
        for k = 1:nc
            n = numel(setup(k).t);
            c = r*nc + k;
            x = setup(k).x0;
            if ~loadPrevious
                x(1) = 1+2*rand;
            end
            x(3) = 4*rand; x(6) = rand; x(2) = 4*rand; x(8:end) = normrnd(0,3,1,n);
            X0(:, c) = 0; X0(1:7+n, c) = x;
            LB(:, c) = LB(:, k); UB(:, c) = UB(:, k); MU(:, c) = MU(:, k); SIG(:, c) = SIG(:, k); J0(:, c) = J0(:, k);
            temper(1, c) = (1/(1 + sqrt(2/(7 + n))))^r;
        end
    end
    keys = repmat(keys, 1, R) + kron(0:R-1, 2^24*ones(1, nc));
    cols = repmat(1:nc, 1, R);
end
sigma2_0 = 1;                                       % :212, :259
MCMCsearch = struct([]);
search = [];
dm = o.demc;
zs = ~isempty(o.demczs);                            % DE-MC(zs): the DE-MC path below, with an archive beside the chains
if zs
    if ~isempty(dm)
        error('tci:demczs', 'demczs and demc are two samplers: give one');
    end
    dm = o.demczs;
    if ~(isnumeric(dm) && numel(dm) == 2 && all(dm == floor(dm)) && dm(1) >= 1 && dm(1) <= 4096 && dm(2) >= 1)
        error('tci:demczs', 'demczs must be [n_pop n_gen] with n_pop in [1, 4096] and n_gen >= 1');
    end
    m0 = max(min(10*P, 4096), max(dm(1), 4));       % the rows of the starting archive
end
n_draw = [];
if ~isempty(dm)
    if zs, n_draw = m0; else, n_draw = dm(1); end   % the members drawn (and searched): the population, or the archive
    if ~zs && ~(isnumeric(dm) && numel(dm) == 2 && all(dm == floor(dm)) && dm(1) >= 4 && dm(1) <= 4096 && dm(2) >= 1)
        error('tci:demc', 'demc must be [n_pop n_gen] with n_pop in [4, 4096] and n_gen >= 1');
    end
    if R > 1 || o.diagnostics || o.logpost || o.stack || o.predict > 0
        error('tci:demc', 'demc cannot be combined with temper, diagnostics, logpost, stack or predict');
    end
    if o.thin <= 0
        error('tci:demc', 'a DE-MC fit is reduced from the kept rows: thin > 0');
    end
    if ~isempty(o.presearch) && o.presearch(1) ~= n_draw
        error('tci:demc', 'presearch n_pop must be the sampler''s n_pop (demczs: its m0 = min(10*P, 4096))');
    end
end
if ~isempty(o.presearch) || ~isempty(dm)            % the mode search: every chain of a cell starts from its best member
    ps = o.presearch;
    if isempty(ps)
        ps = [n_draw 0];                            % DE-MC alone: the population is drawn, not searched
    end
    if ~(isnumeric(ps) && numel(ps) == 2 && all(ps == floor(ps)) && ps(1) >= 4 && ps(1) <= 4096 && ps(2) >= 0)
        error('tci:presearch', 'presearch must be [n_pop n_gen] with n_pop in [4, 4096] and n_gen >= 0');
    end
    n_pop = ps(1);
    POP0 = zeros(P, n_pop*nc);
    for k = 1:nc
        n = numel(setup(k).t);
        POP0(:, (k-1)*n_pop + 1) = X0(:, k);
        for i = 2:n_pop
            x = setup(k).x0;
            if ~loadPrevious
                x(1) = 1+2*rand;
            end
            x(3) = 4*rand; x(6) = rand; x(2) = 4*rand; x(8:end) = normrnd(0,3,1,n);
            POP0(1:7+n, (k-1)*n_pop + i) = x;
        end
    end
    if ~isempty(o.presearch)
        search = tci_mex('modesearch', h, 1:nc, POP0, LB(:, 1:nc), UB(:, 1:nc), MU(:, 1:nc), SIG(:, 1:nc), sigma2_0, ...
            struct('n_gen', ps(2), 'seed', o.seed*1000003 + 20201028, 'keys', [setup.cellNum] - 1));
        for c = 1:numel(cols)
            k = cols(c);
            X0(:, c) = search.pop(:, search.best(k), k);
        end
        POP0 = reshape(search.pop, P, n_pop*nc);
    end
end
if ~isempty(dm)                                     % ---- the DE-MC fit: every output from the members pooled ----
    JIT = 1e-3*sqrt(J0(:, 1:nc));
    for k = 1:nc
        JIT(8+numel(setup(k).t):end, k) = 0;
    end
    dopts = struct('n_gen', dm(2), 'thin', o.thin, 'stats_from', n_burn, 'seed', o.seed*1000003 + 20201028, ...
        'keys', [setup.cellNum] - 1, 'rhat', 1, 'ess', 1, 'rank', double(o.rank ~= 0));
    if zs
        Z0 = POP0;                                  % the archive: the drawn (or searched) population
        n_pop = dm(1);
        C0 = zeros(P, n_pop*nc);                    % the chains: its first rows, or the search's best members
        for k = 1:nc
            pick = 1:n_pop;
            if ~isempty(search)
                [~, order] = sort(search.f(:, k));  % ascending f, ties by index, NaN last
                pick = order(1:n_pop)';
            end
            C0(:, (k-1)*n_pop + (1:n_pop)) = Z0(:, (k-1)*m0 + pick);
        end
        dopts.log_rows = min(dm(2), 1024);
        if ~(ischar(o.bounds) && any(strcmp(o.bounds, {'reject', 'reflect'})))
            error('tci:demczs', 'bounds must be ''reject'' or ''reflect''');
        end
        dopts.bounds = o.bounds;
        dopts.census = double(o.census ~= 0);
        D = tci_mex('demczs', h, 1:nc, C0, Z0, LB(:, 1:nc), UB(:, 1:nc), MU(:, 1:nc), SIG(:, 1:nc), JIT, sigma2_0, dopts);
    else
        D = tci_mex('demc', h, 1:nc, POP0, LB(:, 1:nc), UB(:, 1:nc), MU(:, 1:nc), SIG(:, 1:nc), JIT, sigma2_0, dopts);
    end
    sel = o.thin*(0:size(D.chain, 3)-1) >= n_burn;  % kept row r is generation (r - 1)*thin
    for k = 1:nc
        n = numel(setup(k).t);
        mem = (k-1)*n_pop + (1:n_pop);
        c = reshape(D.chain(1:7+n, mem, sel), 7+n, [])';          % (rows*members) x P, the members of a row together
        s2 = reshape(D.s2chain(mem, sel), [], 1);
        th = mean(c, 1); sd = std(c, 1, 1);
        r.mean_v = th(1);          r.sigma_v = sd(1);
        r.mean_ton = th(3);        r.sigma_ton = sd(3);
        r.mean_A = th(6);          r.sigma_A = sd(6);
        r.mean_tau = th(2);        r.sigma_tau = sd(2);
        r.mean_MS2_basal = th(4);  r.sigma_MS2_basal = sd(4);
        r.mean_PP7_basal = th(5);  r.sigma_PP7_basal = sd(5);
        r.mean_R = th(7);          r.sigma_R = sd(7);
        r.mean_dR = th(8:end);     r.sigma_dR = sd(8:end);
        r.mean_sigma = sqrt(mean(s2));
        r.sigma_sigma = std(sqrt(s2), 1);
        r.cell_index = setup(k).cellNum;
        r.ApprovedFits = setup(k).approved;
        MCMCresults(k) = r;
        [simMS2, simPP7] = tci_mex('forward', h, k, th, 'raw');
        MCMCplot(k) = struct('t_plot', setup(k).t, 'MS2_plot', setup(k).MS2, 'PP7_plot', setup(k).PP7, ...
            'simMS2', simMS2, 'simPP7', simPP7);
        MCMCchain(k) = struct('v_chain', c(:,1), 'ton_chain', c(:,3), 'A_chain', c(:,6), ...
            'tau_chain', c(:,2), 'MS2_basal_chain', c(:,4), 'PP7_basal_chain', c(:,5), ...
            'R_chain', c(:,7), 'dR_chain', c(:,8:end), 's2chain', reshape(D.s2chain(mem, :), [], 1));
        dk = struct('accept_rate', D.accept_rate(:, k)', 'n_oob', D.n_oob(:, k)', 'n_evals', D.n_evals(:, k)', ...
            'rhat_max', D.rhat_max(k), 'ess_min', D.ess_min(k), 'n_pop', n_pop, 'n_gen', dm(2), ...
            'cell_index', setup(k).cellNum);
        if zs
            dk.n_null = D.n_null(:, k)';
            dk.snooker_rate = mean(mean(D.snooker(mem, :)));
            dk.m0 = m0;
            dk.n_archive = D.n_archive;
            if dopts.census
                dk.n_cross = sum(D.n_cross(1:7+n, :, k), 2)';
                dk.oob_lo = sum(D.oob_lo(1:7+n, :, k), 2)';
                dk.oob_hi = sum(D.oob_hi(1:7+n, :, k), 2)';
                dk.oob_share = nan(1, 7+n);
                if strcmp(o.bounds, 'reject') && sum(D.n_oob(:, k)) > 0
                    dk.oob_share = (dk.oob_lo + dk.oob_hi) / sum(D.n_oob(:, k));
                end
            end
            if strcmp(o.bounds, 'reflect')
                dk.reflect_rate = sum(D.n_reflected(:, k)) / (n_pop*dm(2));
            end
            if isempty(MCMCdemczs), MCMCdemczs = dk; else, MCMCdemczs(k) = dk; end
        else
            if isempty(MCMCdemc), MCMCdemc = dk; else, MCMCdemc(k) = dk; end
        end
        if o.rank
            rk = rank_entry(D.rank, k, n, setup(k).cellNum);
            if isempty(MCMCrank), MCMCrank = rk; else, MCMCrank(k) = rk; end
        end
        if ~isempty(search)
            qk = struct('f_best', search.f_best(k), 'ss_best', search.ss_best(k), 'theta_best', search.theta_best(1:7+n, k)', ...
                'f0_best', search.f_trace(k, 1), 'f_trace', search.f_trace(k, :), 'n_gen', size(search.f_trace, 2) - 1, ...
                'n_pop', size(search.pop, 2), 'n_evals', size(search.pop, 2)*size(search.f_trace, 2), ...
                'cell_index', setup(k).cellNum);
            if isempty(MCMCsearch), MCMCsearch = qk; else, MCMCsearch(k) = qk; end
        end
    end
    return
end
options = struct('nsimu', n_steps, 'burnintime', n_burn, 'adaptint', 100, 'method', 'dram', ...  % :263-270
    'updatesigma', 1, 'verbosity', 0, 'stats_from', max(n_burn, 1), 'thin', o.thin, ...
    'seed', o.seed*1000003 + 20201028, 'engine', o.engine, 'adapt_pmax', o.adapt_pmax, ...
    'chain_keys', keys);
MCMCtemper = struct([]);
if R > 1
    options.temper = temper;
    options.swap_every = o.swap_every;
end
MCMCdiag = struct([]);
MCMClp = struct([]);
if o.logpost && o.thin <= 0
    error('tci:logpost', 'the log-posterior trace needs the kept chain rows: thin > 0');
end
if o.logpost
    options.logpost = 1;
end
MCMCstack = struct([]);
if o.stack && o.thin <= 0
    error('tci:stack', 'PSIS-LOO needs the kept chain rows: thin > 0');
end
if o.stack
    options.stack = o.stack;
end
if o.rank
    if R > 1 || o.logpost
        error('tci:rank', 'rank cannot be combined with temper or logpost');
    end
    options.rank = 1;
end
if o.diagnostics && o.thin <= 0
    error('tci:diagnostics', 'the diagnostics need the kept chain rows: thin > 0');
end
if o.diagnostics
    [results, chain, s2chain, ~, stats] = tci_mex('dram', h, cols, X0, LB, UB, MU, SIG, J0, sigma2_0, options);
    rows = 1 + o.thin*(0:size(chain, 3)-1);
    sel = rows >= max(n_burn, 1);
elseif o.thin > 0
    [results, chain, s2chain] = tci_mex('dram', h, cols, X0, LB, UB, MU, SIG, J0, sigma2_0, options);  % :273
    rows = 1 + o.thin*(0:size(chain, 3)-1);         % chain rows kept: 1, 1+thin, ...
    sel = rows >= max(n_burn, 1);                   % chain(n_burn:end, :) (:276-283)
else
    results = tci_mex('dram', h, cols, X0, LB, UB, MU, SIG, J0, sigma2_0, options);
end

% ---- predictive bands: the same sample rows for every cell, one call (mcmcpred, deterministic rows) --
if o.predict > 0
    kept = find(sel);
    if isempty(kept)
        error('tci:predict', 'the fit kept no chain rows after n_burn');
    end
    if numel(kept) >= o.predict
        kept = kept(round(linspace(1, numel(kept), o.predict)));
    end
    pred_probs = [0.025, 0.5, 0.975];
    [predMS2, predPP7] = tci_mex('predict', h, 1:nc, permute(chain(:, :, kept), [1 3 2]), pred_probs, 'raw');
end

% ---- summaries, forward model at the means, the three structs (:276-356) -------------------------
for k = 1:nc
    n = numel(setup(k).t);
    th = results.mean(1:7+n, k)';
    sd = results.std(1:7+n, k)';
    r.mean_v = th(1);          r.sigma_v = sd(1);   % :286-301 (std(., 1))
    r.mean_ton = th(3);        r.sigma_ton = sd(3);
    r.mean_A = th(6);          r.sigma_A = sd(6);
    r.mean_tau = th(2);        r.sigma_tau = sd(2);
    r.mean_MS2_basal = th(4);  r.sigma_MS2_basal = sd(4);
    r.mean_PP7_basal = th(5);  r.sigma_PP7_basal = sd(5);
    r.mean_R = th(7);          r.sigma_R = sd(7);
    r.mean_dR = th(8:end);     r.sigma_dR = sd(8:end);
    r.mean_sigma = results.sigma_mean(k);           % :302-303
    r.sigma_sigma = results.sigma_std(k);
    r.cell_index = setup(k).cellNum;                  % :343
    r.ApprovedFits = setup(k).approved;               % :345-350
    MCMCresults(k) = r;
    [simMS2, simPP7] = tci_mex('forward', h, k, th, 'raw');   % :307-309 (x mean_A inside)
    plotk = struct('t_plot', setup(k).t, 'MS2_plot', setup(k).MS2, 'PP7_plot', setup(k).PP7, ...
        'simMS2', simMS2, 'simPP7', simPP7);
    if o.predict > 0
        plotk.predMS2 = predMS2(1:n, :, k)';            % nq x N
        plotk.predPP7 = predPP7(1:n, :, k)';
        plotk.pred_probs = pred_probs;
    end
    MCMCplot(k) = plotk;
    if o.diagnostics
        names = {'v', 'ton', 'A', 'tau', 'MS2_basal', 'PP7_basal', 'R'};
        col = [1 3 6 2 4 5 7];
        src = {'mcerr', stats.mcerr, stats.s2_mcerr; 'tau', stats.tau, stats.s2_tau; ...
               'geweke_p', stats.geweke_p, stats.s2_geweke_p};
        dg = struct();
        for q = 1:3
            for w = 1:7
                dg.([src{q, 1} '_' names{w}]) = src{q, 2}(col(w), k);
            end
            dg.([src{q, 1} '_dR']) = src{q, 2}(8:7+n, k)';
            dg.([src{q, 1} '_s2']) = src{q, 3}(k);
        end
        dg.n_rows = stats.n_rows;
        dg.ess_min = stats.n_rows / max(stats.tau(1:7+n, k));
        dg.cell_index = setup(k).cellNum;
        if isempty(MCMCdiag), MCMCdiag = dg; else, MCMCdiag(k) = dg; end
    end
    if o.logpost
        L = results.logpost;
        lpk = struct('ss', L.ss(k, :)', 'lp', L.lp(k, :)');
        for f = {'ss_min', 'ss_mean', 'dev_mean', 'dev_var', 'best_row', 'lp_best', 'ss_best', 's2_best', ...
                 's2_mean', 'ss_hat', 'd_hat', 'p_d', 'p_v', 'dic'}
            lpk.(f{1}) = L.(f{1})(k);
        end
        names = {'v', 'ton', 'A', 'tau', 'MS2_basal', 'PP7_basal', 'R'};
        col = [1 3 6 2 4 5 7];
        for w = 1:7
            lpk.(['best_' names{w}]) = L.theta_best(col(w), k);
        end
        lpk.best_dR = L.theta_best(8:7+n, k)';
        lpk.n_rows = L.n_rows;
        lpk.cell_index = setup(k).cellNum;
        if isempty(MCMClp), MCMClp = lpk; else, MCMClp(k) = lpk; end
    end
    if o.stack
        T = results.stack;
        g = T.group(k);
        sk = struct('weights', T.weight(k), 'elpd_loo', T.elpd_loo(k), 'p_loo', T.p_loo(k), ...
            'khat_max', T.khat_max(k), 'n_khat_bad', T.n_khat_bad(k), 'elpd_loo_i', T.elpd_loo_i(1:n, :, k)', ...
            'khat_i', T.khat_i(1:n, :, k)', 'elpd_stack', T.elpd_stack(g), ...
            'stacked_mean', T.weight(k)*results.mean(1:7+n, k)', 'n_samples', numel(T.rows), ...
            'cell_index', setup(k).cellNum);
        if isempty(MCMCstack), MCMCstack = sk; else, MCMCstack(k) = sk; end
    end
    if o.rank
        rk = rank_entry(results.rank, results.rank.group(k), n, setup(k).cellNum);
        if isempty(MCMCrank), MCMCrank = rk; else, MCMCrank(k) = rk; end
    end
    if ~isempty(search)
        qk = struct('f_best', search.f_best(k), 'ss_best', search.ss_best(k), 'theta_best', search.theta_best(1:7+n, k)', ...
            'f0_best', search.f_trace(k, 1), 'f_trace', search.f_trace(k, :), 'n_gen', size(search.f_trace, 2) - 1, ...
            'n_pop', size(search.pop, 2), 'n_evals', size(search.pop, 2)*size(search.f_trace, 2), ...
            'cell_index', setup(k).cellNum);
        if isempty(MCMCsearch), MCMCsearch = qk; else, MCMCsearch(k) = qk; end
    end
    if R > 1
        T = results.temper;
        rungs = k + nc*(0:R-1);
        tk = struct('beta', T.beta(rungs), 'swap_rate', T.swap_accepted(rungs(1:end-1)) ./ T.swap_tried(rungs(1:end-1)), ...
            'swap_tried', T.swap_tried(rungs(1:end-1)), 'accept_rate', results.accept_rate(rungs), ...
            'swap_every', T.swap_every, 'n_events', T.n_events, 'cell_index', setup(k).cellNum);
        if isempty(MCMCtemper), MCMCtemper = tk; else, MCMCtemper(k) = tk; end
    end
    if o.thin > 0
        c = reshape(chain(1:7+n, k, sel), 7+n, [])';   % rows x P
        MCMCchain(k) = struct('v_chain', c(:,1), 'ton_chain', c(:,3), 'A_chain', c(:,6), ...
            'tau_chain', c(:,2), 'MS2_basal_chain', c(:,4), 'PP7_basal_chain', c(:,5), ...
            'R_chain', c(:,7), 'dR_chain', c(:,8:end), 's2chain', s2chain(k, :)');   % :315-323
    else
        MCMCchain(k) = struct('v_chain', [], 'ton_chain', [], 'A_chain', [], 'tau_chain', [], ...
            'MS2_basal_chain', [], 'PP7_basal_chain', [], 'R_chain', [], 'dR_chain', [], 's2chain', []);
    end
end
end

function rk = rank_entry(K, g, n, cellNum)
% One MCMCrank entry from group g of res.rank of tci_mex('dram') / tci_mex('demc'), a cell of n points: the vectors
% trimmed to the cell's 7 + n parameters with sigma2 appended as the last column.
rk = struct('q', [K.q(1:7+n, :, g)', K.s2_q(:, g)], 'q_tail', [K.q_tail(1:7+n, :, g)', K.s2_q_tail(:, g)]);
for f = {'rhat_bulk', 'rhat_folded', 'rhat_rank', 'ess_bulk', 'tau_bulk', 'ess_tail_lo', 'ess_tail_hi', 'ess_tail', ...
         'window_bulk', 'window_tail_lo', 'window_tail_hi'}
    rk.(f{1}) = [K.(f{1})(1:7+n, g)', K.(['s2_' f{1}])(g)];
end
rk.n_rows = K.n_rows;
rk.cell_index = cellNum;
end
