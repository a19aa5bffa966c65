// Robust linear regression: a Student-t likelihood with nu = 4 degrees of freedom (a literal), normal(0, s)
// priors on alpha and beta, flat on sigma.
data {
  int<lower=0> N;
  int<lower=0> K;
  matrix[N, K] x;
  vector[N] y;
}
parameters {
  real alpha;
  vector[K] beta;
  real<lower=0> sigma;
}
model {
  alpha ~ normal(0, 10);
  beta ~ normal(0, 2.5);
  y ~ student_t(4, alpha + x * beta, sigma);
}
