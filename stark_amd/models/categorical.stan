// Softmax regression with ncat classes, class ncat the reference (eta = 0), flat priors.  beta is a column-major
// vector: class g's coefficients are beta[(g - 1) K + 1 .. g K].
data {
  int<lower=0> N;
  int<lower=1> K;
  int<lower=2> ncat;
  matrix[N, K] x;
  int<lower=1, upper=ncat> y[N];
}
parameters {
  vector[ncat - 1] alpha;
  vector[K * (ncat - 1)] beta;
}
model {
  matrix[N, ncat - 1] eta = rep_matrix(alpha', N) + x * to_matrix(beta, K, ncat - 1);
  for (n in 1:N) y[n] ~ categorical_logit(append_row(eta[n]', 0));
}
