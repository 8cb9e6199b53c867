"""TEST INFRASTRUCTURE -- numpy restatement of the reference's identification block with the order PN as a parameter
(README.md:116-153), op for op:
    for i = PN+1:num_train: AA(i-PN, n*(j-1)+1 : n*j) = ad_acc(i-j, :) (j = 1..PN) ;  BB(i-PN, :) = ad_acc(i, :)
    PARA = (AA'*AA) \\ AA'*BB ;  A_j = PARA(n*(j-1)+1 : n*j, :)'
    for i = 1:num_test: AA_valid(i, n*(j-1)+1 : n*j) = ad_acc(i+num_train-j, :) ;  BB_valid(i, :) = ad_acc(i+num_train, :)
    RMSE_valid(q) = sqrt(mean((AA_valid*PARA - BB_valid)(:, q).^2)) ;  RRMSE_valid(q) = RMSE_valid(q) / (max - min)(BB_valid(:, q))
PARITY UNPINNED (the reference is MATLAB only and ships neither the data set nor outputs).  Checker only."""
import numpy as np


def design(ad_acc, num_train, PN):
    ad = np.asarray(ad_acc, dtype=np.float64)
    n = ad.shape[1]
    AA = np.zeros((num_train - PN, PN * n)); BB = np.zeros((num_train - PN, n))
    for i in range(PN, num_train):                 # MATLAB i = PN+1 .. num_train (1-based)
        for j in range(1, PN + 1):
            AA[i - PN, n * (j - 1):n * j] = ad[i - j]
        BB[i - PN] = ad[i]
    return AA, BB


def identify_var(ad_acc, num_train, PN):
    """Returns ([A_1 .. A_PN], cond_2(AA'AA))."""
    AA, BB = design(ad_acc, num_train, PN)
    n = BB.shape[1]
    G = AA.T @ AA
    PARA = np.linalg.solve(G, AA.T @ BB)
    return [PARA[n * j:n * (j + 1)].T.copy() for j in range(PN)], float(np.linalg.cond(G))


def validate_var(ad_acc, A, num_train, num_test):
    """A: the list [A_1 .. A_PN].  Returns (RMSE_valid, RRMSE_valid) without the reference's leading piston zero."""
    ad = np.asarray(ad_acc, dtype=np.float64)
    n = ad.shape[1]
    PN = len(A)
    PARA = np.concatenate([np.asarray(Aj).T for Aj in A], axis=0)
    AAv = np.zeros((num_test, PN * n)); BBv = np.zeros((num_test, n))
    for i in range(1, num_test + 1):               # MATLAB i = 1 .. num_test; row i+num_train (1-based) = index i+num_train-1
        for j in range(1, PN + 1):
            AAv[i - 1, n * (j - 1):n * j] = ad[i + num_train - j - 1]
        BBv[i - 1] = ad[i + num_train - 1]
    pred = AAv @ PARA
    rmse = np.sqrt(np.mean((pred - BBv) ** 2, axis=0))
    with np.errstate(divide="ignore", invalid="ignore"):
        rrmse = rmse / (BBv.max(axis=0) - BBv.min(axis=0))
    return rmse, rrmse
