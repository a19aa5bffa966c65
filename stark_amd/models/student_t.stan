// Robust linear regression: a Student-t likelihood with nu degrees of freedom (data, never a parameter),
// flat priors on alpha, beta and sigma.
data {
  int<lower=0> N;
  int<lower=0> K;
  matrix[N, K] x;
  vector[N] y;
  real<lower=0> nu;
}
parameters {
  real alpha;
  vector[K] beta;
  real<lower=0> sigma;
}
model {
  y ~ student_t(nu, alpha + x * beta, sigma);
}
